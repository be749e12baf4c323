// kernels_query.hip -- ivfflatgettuple's data path for ONE query, nothing but the head read back.
//
// A Postgres backend scans an index for one query at a time (src/ivfscan.c:361-414): the first
// amgettuple call runs GetScanLists (:47-118), then GetScanItems (:123-187) scores every tuple of
// the next `probes` lists and sorts them, and the executor usually pulls only LIMIT k of them.
// The batched path (plan kernels + tile scan + segmented top-k) needs ~10 launches and two host
// round trips for that; here it is a chain of four small launches on one queue with no host
// involvement in between (five where the device is not behind a large PCIe BAR):
//
//   (the host stores the padded query straight into a fine-grained device row: hipDeviceAttributeIsLargeBar;
//    otherwise query_stage_kernel copies it from pinned host memory -- one more launch, ~2 us)
//   query_rank_kernel    distance to every center, spread over all CUs
//   query_lists_kernel   the max_probes nearest (ascending, lower id on ties) -> device memory
//   query_scan_kernel    the ~N*probes/lists rows of the next `probes` lists split evenly over all
//                        workgroups (rows are ~6 KB, a wavefront keeps two in flight): pure
//                        streaming, distances kept in HBM in tuplesort input order
//   query_head_kernel    selects and sorts the head of the stream and writes (distance, slot, tid)
//                        into pinned host memory, the sequence word last -- no list of 10 000
//                        distances crosses PCIe, no host sort, no stream synchronise
//
// A dependent kernel boundary costs ~1.5 us on this chip (MI355X_MICROARCH.md price list), less
// than an in-kernel "last workgroup selects" hand-off (write-through stores, drain, ~1500 tickets,
// acquire: ~5 us measured), and it keeps the scan kernel a clean streaming kernel.
//
// pgv_rank_lists / pgv_search_batch for a few queries launch the same rank, lists and scan kernels with a grid row per
// query, and mq_head_kernel in place of query_head_kernel: heads into device arrays, no pinned record.
#include "pgv_device.h"
#include "pgv_select.h"

#include <type_traits>

namespace pgv {

namespace {

constexpr int kQThreads = kSelThreads;  // 256: block_topk's geometry
constexpr int kQWaves = kQThreads / kWave;
constexpr int kMaxBatchLists = 256;     // probes per GetScanItems batch the fused path handles
constexpr int kHeadCap = 1024;          // entries block_topk may keep

// ---- scoring: rows of whole 1 KiB slices keep the query in registers and two rows in flight
template <typename T, int METRIC, int NCH> struct WholeRows {
    Raw16 q[NCH];
    __device__ __forceinline__ void load_query(const char *qp, int lane) {
#pragma unroll
        for (int c = 0; c < NCH; c++) q[c] = load16(qp + ((size_t)c * kWave + lane) * sizeof(Raw16));
    }
    // distances of rows a and b: even lanes return a's, odd lanes b's
    __device__ __forceinline__ float pair(const char *a, const char *b, int lane) const {
        Raw16 ra[NCH], rb[NCH];
#pragma unroll
        for (int c = 0; c < NCH; c++) ra[c] = load16(a + ((size_t)c * kWave + lane) * sizeof(Raw16));
#pragma unroll
        for (int c = 0; c < NCH; c++) rb[c] = load16(b + ((size_t)c * kWave + lane) * sizeof(Raw16));
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; c++) sa = accum_slice<T, METRIC>(sa, ra[c], q[c]);
#pragma unroll
        for (int c = 0; c < NCH; c++) sb = accum_slice<T, METRIC>(sb, rb[c], q[c]);
        return finish<METRIC>(wave_sum2(sa, sb));
    }
};

// any row length: 1 << lg lanes per row, 64 >> lg rows per wavefront step; the total is valid
// in the last lane of each group
template <typename T, int METRIC>
__device__ __forceinline__ float group_distance(const char *row, const char *qp, int nvec, int lane_in, int lg) {
    const int lpr = 1 << lg;
    float acc0 = 0.f, acc1 = 0.f;
    int v = lane_in;
    for (; v + lpr < nvec; v += 2 * lpr) {
        const Raw16 a0 = load16(row + (size_t)v * sizeof(Raw16));
        const Raw16 a1 = load16(row + (size_t)(v + lpr) * sizeof(Raw16));
        acc0 = accum_slice<T, METRIC>(acc0, a0, load16(qp + (size_t)v * sizeof(Raw16)));
        acc1 = accum_slice<T, METRIC>(acc1, a1, load16(qp + (size_t)(v + lpr) * sizeof(Raw16)));
    }
    if (v < nvec) acc0 = accum_slice<T, METRIC>(acc0, load16(row + (size_t)v * sizeof(Raw16)), load16(qp + (size_t)v * sizeof(Raw16)));
    return finish<METRIC>(group_sum_to_last(acc0 + acc1, lg));
}

// group_distance<float, 0> and, over the same loads, the inner product q.row in two accumulators of its own (the pair
// terms of the shadow scan, pgv_internal.h: pair_chain_length).  The chain of sum((q - x)^2) is group_distance's
// operation for operation: its value does not change by a bit.
__device__ __forceinline__ float group_distance_dot(const char *row, const char *qp, int nvec, int lane_in, int lg, float *dot) {
    const int lpr = 1 << lg;
    float acc0 = 0.f, acc1 = 0.f, dot0 = 0.f, dot1 = 0.f;
    int v = lane_in;
    for (; v + lpr < nvec; v += 2 * lpr) {
        const Raw16 a0 = load16(row + (size_t)v * sizeof(Raw16));
        const Raw16 a1 = load16(row + (size_t)(v + lpr) * sizeof(Raw16));
        const Raw16 q0 = load16(qp + (size_t)v * sizeof(Raw16));
        const Raw16 q1 = load16(qp + (size_t)(v + lpr) * sizeof(Raw16));
        acc0 = accum_slice<float, 0>(acc0, a0, q0);
        acc1 = accum_slice<float, 0>(acc1, a1, q1);
        dot0 = accum_slice<float, 1>(dot0, a0, q0);
        dot1 = accum_slice<float, 1>(dot1, a1, q1);
    }
    if (v < nvec) {
        const Raw16 a0 = load16(row + (size_t)v * sizeof(Raw16)), q0 = load16(qp + (size_t)v * sizeof(Raw16));
        acc0 = accum_slice<float, 0>(acc0, a0, q0);
        dot0 = accum_slice<float, 1>(dot0, a0, q0);
    }
    *dot = group_sum_to_last(dot0 + dot1, lg);
    return finish<0>(group_sum_to_last(acc0 + acc1, lg));
}

// score_rows<float, 0, 0> with q.row of every row to out_dot[j] beside the distance
template <typename RowPtr>
__device__ __forceinline__ void score_rows_dot(RowPtr row_ptr, int64_t first, int64_t end, const char *qp, int nvec, int lg,
                                               float *out, float *out_dot) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int rpw = kWave >> lg;  // rows per wavefront step
    const int g = lane >> lg, lane_in = lane & ((1 << lg) - 1);
    for (int64_t j0 = first + (int64_t)wave * rpw; j0 < end; j0 += (int64_t)kQWaves * rpw) {
        const int64_t j = j0 + g;
        const bool valid = j < end;
        float dot;
        const float d = group_distance_dot(row_ptr(valid ? j : end - 1), qp, nvec, lane_in, lg, &dot);
        if (valid && lane_in == (1 << lg) - 1) {
            out[j] = d;
            out_dot[j] = dot;
        }
    }
}

// t = -2 q.row of the k rows a query's output row names (slot < 0: none, t = 0), one wavefront per row with
// shadow_pair_kernel's chain: a flagged query of the ranking, whose lists batch_fix_kernel has just decided
__device__ __forceinline__ void fill_pair_terms(const char *vectors, size_t row_bytes, const char *qrow, int ld,
                                                const int32_t *slots_i32, const int64_t *slots_i64, int k,
                                                float *__restrict__ pair_t) {
    const int lane = threadIdx.x & (kWave - 1);
    for (int i = threadIdx.x >> 6; i < k; i += kQWaves) {
        // (written by this workgroup's other wavefronts a moment ago, before a barrier: agent-scope loads)
        const int64_t slot = slots_i32 ? (int64_t)__hip_atomic_load(slots_i32 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                       : __hip_atomic_load(slots_i64 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        float a = 0.f;
        if (slot >= 0) {
            const float *x = reinterpret_cast<const float *>(qrow);
            const float *c = reinterpret_cast<const float *>(vectors + (size_t)slot * row_bytes);
            for (int e = lane; e < ld; e += kWave) a = fmaf(x[e], c[e], a);
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        }
        if (lane == 0) pair_t[i] = -2.f * a;
    }
}

// rows [first, end) given by a functor row_ptr(j) -> const char*, distances to out[j]
template <typename T, int METRIC, int NCH, typename RowPtr>
__device__ __forceinline__ void score_rows(RowPtr row_ptr, int64_t first, int64_t end, const char *qp, int nvec, int lg,
                                           float *out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    if constexpr (NCH > 0) {
        WholeRows<T, METRIC, NCH> w;
        w.load_query(qp, lane);
        for (int64_t j = first + 2 * wave; j < end; j += 2 * kQWaves) {
            const bool two = j + 1 < end;
            const float d = w.pair(row_ptr(j), row_ptr(two ? j + 1 : j), lane);
            if (lane == 0 || (lane == 1 && two)) out[j + lane] = d;
        }
    } else {
        const int rpw = kWave >> lg;  // rows per wavefront step
        const int g = lane >> lg, lane_in = lane & ((1 << lg) - 1);
        for (int64_t j0 = first + (int64_t)wave * rpw; j0 < end; j0 += (int64_t)kQWaves * rpw) {
            const int64_t j = j0 + g;
            const bool valid = j < end;
            const float d = group_distance<T, METRIC>(row_ptr(valid ? j : end - 1), qp, nvec, lane_in, lg);
            if (valid && lane_in == (1 << lg) - 1) out[j] = d;
        }
    }
}

// The rank, lists and scan kernels take one query per grid row: the single-query entry points launch one row, a batch
// too small to share rows between its queries (nq * probes well below the list count: every probed list belongs to one
// query, the list-major plan of the batched path gains nothing and pays its dozen launches) launches nq of them.
// ------------------------------------------------------------------- GetScanLists
// grid row q (blockIdx.y): query q of `queries` against every center, distances to cdist[q * cd_stride + list]
template <typename T, int METRIC, int NCH>
__global__ __launch_bounds__(kQThreads) void query_rank_kernel(const char *__restrict__ centers, int nlists, int nvec,
                                                               int lg, const char *__restrict__ queries,
                                                               float *__restrict__ cdist, int64_t cd_stride, int per) {
    const size_t row_bytes = (size_t)nvec * sizeof(Raw16);
    const char *qp = queries + (size_t)blockIdx.y * row_bytes;
    float *cd = cdist + (size_t)blockIdx.y * cd_stride;
    for (int64_t first = (int64_t)blockIdx.x * per; first < nlists; first += (int64_t)gridDim.x * per) {
        const int64_t end = first + per < nlists ? first + per : nlists;
        score_rows<T, METRIC, NCH>([&](int64_t j) { return centers + (size_t)j * row_bytes; }, first, end, qp, nvec, lg, cd);
    }
}

// the bounded heap of GetScanLists (src/ivfscan.c:76-106): max_probes nearest centers, ascending; one workgroup per
// query (blockIdx.x), out_dist optional
__global__ __launch_bounds__(kQThreads) void query_lists_kernel(const float *__restrict__ cdist, int64_t cd_stride,
                                                                int nlists, int max_probes, int kp,
                                                                int32_t *__restrict__ out_lists,
                                                                float *__restrict__ out_dist) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long *ent = reinterpret_cast<unsigned long long *>(smem);
    SelShared *s = reinterpret_cast<SelShared *>(smem + (size_t)kHeadCap * 8);
    const int q = blockIdx.x;
    block_topk_auto(cdist + (size_t)q * cd_stride, nlists, max_probes, kp, kHeadCap, ent, s);
    for (int i = threadIdx.x; i < max_probes; i += kQThreads) {
        out_lists[(size_t)q * max_probes + i] = (int32_t)(unsigned)(ent[i] & 0xffffffffu);
        if (out_dist) out_dist[(size_t)q * max_probes + i] = key_to_float((unsigned)(ent[i] >> 32));
    }
}

// ------------------------------------------------------------------- GetScanItems
// where each probed list starts in the batch (offs) and its first row slot (lbeg): lists in probe
// order, page-chain order inside -- the order the reference feeds its tuplesort
struct BatchMap {
    int64_t offs[kMaxBatchLists + 1];
    int64_t lbeg[kMaxBatchLists];
    __device__ void build(const int32_t *probe_lists, int nprobes, const int64_t *list_off) {
        if ((int)threadIdx.x < nprobes) {
            const int l = probe_lists[threadIdx.x];
            lbeg[threadIdx.x] = list_off[l];
            offs[threadIdx.x + 1] = list_off[l + 1] - list_off[l];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            offs[0] = 0;
            for (int p = 0; p < nprobes; p++) offs[p + 1] += offs[p];
        }
        __syncthreads();
    }
    __device__ __forceinline__ int64_t slot_of(int64_t j, int nprobes) const {  // batch position -> row slot
        int lo = 0, hi = nprobes - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (offs[mid] <= j)
                lo = mid;
            else
                hi = mid - 1;
        }
        return lbeg[lo] + (j - offs[lo]);
    }
};

// grid row q (blockIdx.y): query q over its own nprobes lists, distances to seg[q * seg_stride + position in the batch]
template <typename T, int METRIC, int NCH>
__global__ __launch_bounds__(kQThreads) void query_scan_kernel(
    const char *__restrict__ vectors, const int64_t *__restrict__ list_off, const int32_t *__restrict__ probe_lists,
    int nprobes, int nvec, int lg, const char *__restrict__ queries, float *__restrict__ seg, int64_t seg_stride, int per) {
    __shared__ BatchMap map;
    const size_t row_bytes = (size_t)nvec * sizeof(Raw16);
    const int q = blockIdx.y;
    map.build(probe_lists + (size_t)q * nprobes, nprobes, list_off);
    const int64_t m = map.offs[nprobes];
    const char *qp = queries + (size_t)q * row_bytes;
    float *sg = seg + (size_t)q * seg_stride;
    if (!queries) {
        // NULL query (pgv_query_scan alone hands one in): ZeroDistance (src/ivfscan.c:192-196), every tuple at distance
        // 0.  In front of the scoring loop: as a branch inside it, this cost the six-slice kernel 10 VGPRs and a wave
        // per SIMD
        for (int64_t j = (int64_t)blockIdx.x * kQThreads + threadIdx.x; j < m; j += (int64_t)gridDim.x * kQThreads) sg[j] = 0.f;
        return;
    }
    // runs of `per` rows per workgroup, round-robin until the batch is covered (the grid was sized
    // from the host's upper bound of m)
    for (int64_t first = (int64_t)blockIdx.x * per; first < m; first += (int64_t)gridDim.x * per) {
        const int64_t end = first + per < m ? first + per : m;
        score_rows<T, METRIC, NCH>([&](int64_t j) { return vectors + (size_t)map.slot_of(j, nprobes) * row_bytes; }, first,
                                   end, qp, nvec, lg, sg);
    }
}

// What the two head kernels share: the map of the batch and the first k entries of its ascending tuplesort stream
// (distance, then position) into ent[0, min(k, m)) at the start of smem.  Returns m, the tuples of the batch.
__device__ __forceinline__ int64_t select_head(BatchMap &map, char *smem, const float *seg, const int64_t *list_off,
                                               const int32_t *probe_lists, int nprobes, int k, int kp) {
    map.build(probe_lists, nprobes, list_off);
    const int64_t m = map.offs[nprobes];
    block_topk_auto(seg, m, k, kp, kHeadCap, reinterpret_cast<unsigned long long *>(smem),
                    reinterpret_cast<SelShared *>(smem + (size_t)kHeadCap * 8));
    return m;
}

// entries [skip, skip + count) of the ascending tuplesort stream of the batch whose distances are
// in seg[0, m) (tuplesort_performsort + the executor's pulls, src/ivfscan.c:182, :408-413): the
// head right after the scan (skip = 0), deeper windows when the executor pulls on (one workgroup;
// k = skip + count <= kHeadCap).  Results go to pinned host memory, the sequence word last.
__global__ __launch_bounds__(kQThreads) void query_head_kernel(
    const float *__restrict__ seg, const int64_t *__restrict__ list_off, const uint64_t *__restrict__ tids,
    const int32_t *__restrict__ probe_lists, int nprobes, int skip, int count, int kp, QueryHead *__restrict__ hdr,
    float *__restrict__ head_dist, int64_t *__restrict__ head_slot, uint64_t *__restrict__ head_tid, unsigned seq) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ BatchMap map;
    const int k = skip + count;
    const int64_t m = select_head(map, smem, seg, list_off, probe_lists, nprobes, k, kp);
    const unsigned long long *ent = reinterpret_cast<const unsigned long long *>(smem);
    const int have = (int)(m < k ? m : k) - skip;
    for (int i = threadIdx.x; i < have; i += kQThreads) {
        const unsigned long long e = ent[skip + i];
        const int64_t slot = map.slot_of((int64_t)(unsigned)(e & 0xffffffffu), nprobes);
        head_dist[i] = key_to_float((unsigned)(e >> 32));
        head_slot[i] = slot;
        head_tid[i] = tids ? tids[slot] : ~0ull;
    }
    // every wavefront's stores have left before the record is declared complete; the host polls seq
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        hdr->total = m;
        hdr->count = have > 0 ? have : 0;
        __hip_atomic_store(&hdr->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// the query payload from pinned host memory into its padded device row (one launch on the same
// queue instead of a copy-engine transfer with its cross-queue hand-off)
// (the host side has already padded it: whole 16-byte vectors, one PCIe round trip per thread)
__global__ __launch_bounds__(1024) void query_stage_kernel(const Raw16 *__restrict__ src, Raw16 *__restrict__ dst, int nvec) {
    for (int i = threadIdx.x; i < nvec; i += 1024) dst[i] = src[i];
}

// NULL query: ZeroDistance ranks the first max_probes lists (strict `<` never replaces, src/ivfscan.c:92)
__global__ void query_iota_kernel(int32_t *__restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}

// a few queries at a time: the head of each query's stream (one workgroup per query) into the caller's [nq x k] device
// arrays (+inf / -1 / ~0 past the tuples there are) -- with rank, lists and scan pgv_search_batch for 16 queries in
// four launches
__global__ __launch_bounds__(kQThreads) void mq_head_kernel(
    const float *__restrict__ seg, int64_t seg_stride, const int64_t *__restrict__ list_off,
    const uint64_t *__restrict__ tids, const int32_t *__restrict__ probe_lists, int nprobes, int k, int kp,
    float *__restrict__ out_dist, int64_t *__restrict__ out_slot, uint64_t *__restrict__ out_tid,
    double *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ BatchMap map;
    const int q = blockIdx.x;
    const int64_t m = select_head(map, smem, seg + (size_t)q * seg_stride, list_off, probe_lists + (size_t)q * nprobes,
                                  nprobes, k, kp);
    const unsigned long long *ent = reinterpret_cast<const unsigned long long *>(smem);
    const int have = (int)(m < k ? m : k);
    for (int i = threadIdx.x; i < k; i += kQThreads) {
        const size_t o = (size_t)q * k + i;
        if (i < have) {
            const unsigned long long e = ent[i];
            const int64_t slot = map.slot_of((int64_t)(unsigned)(e & 0xffffffffu), nprobes);
            out_dist[o] = key_to_float((unsigned)(e >> 32));
            if (out_slot) out_slot[o] = slot;
            if (out_tid) out_tid[o] = tids ? tids[slot] : ~0ull;
        } else {
            out_dist[o] = INFINITY;
            if (out_slot) out_slot[o] = -1;
            if (out_tid) out_tid[o] = ~0ull;
        }
    }
    if (stats && threadIdx.x == 0) {  // profiling: pairs scored = rows streamed = rows of probed lists (nothing is shared)
        atomicAdd(&stats[0], (double)m);
        atomicAdd(&stats[1], (double)m);
        atomicAdd(&stats[5], (double)m);
    }
}

// ------------------------------------------------------------------- exact tail of the MFMA L2 scan
// mfma_scan_kernel's L2 values are |x|^2 - 2 q.x (the expansion of the distance less its per-query constant |q|^2):
// they pick k' candidates per query, and this
// kernel (one workgroup per query) re-evaluates those with the reference's arithmetic
// (sum of (q - x)^2, src/vector.c:172-185), sorts them the way the tuplesort would (distance, then
// position in the stream) and emits the first k.  A query is flagged for the full exact pass unless
// the k'-th approximate value clears the k-th one by twice the rounding bound of the expansion, i.e.
// unless no row outside the candidates can belong to the head.
constexpr int kRecheckCap = 256;  // k' <= 256: rank_sort_entries' reach

// Probe pruning (the rule and its proof: pgv_internal.h, beside ScanBound) as the workgroup of one query runs it, called
// by every thread: the thread of probe j (j < 0: none; !live: a fill entry, no list) brings the probe's exact center
// distance d and its list's radius r, lens[0 .. n) hold the probed lists' rows in probe order (written before the call,
// 0 for a fill entry), near[n] is scratch.  Returns
// 2 * (probes dropped in the workgroup) + (this thread's probe is dropped)
__device__ __forceinline__ int probe_prune_step(const int64_t *lens, double *near, int n, int j, bool live, float d, float r,
                                                int need, int ld) {
    const ProbeMargins pm = probe_margins(ld);
    if (j >= 0) near[j] = live ? probe_near(d, r, pm) : 0.0;
    __syncthreads();
    const bool drop = j >= 0 && live && probe_dropped(lens, near, n, j, need, probe_far(d, r, pm), pm);
    return 2 * __syncthreads_count(drop) + (drop ? 1 : 0);
}
// ... out of line for batch_fix_kernel, whose registers its selection forms fill: inlined twice (both ends of a flagged
// query), the fp64 square roots and divisions cost it a wave per SIMD
__device__ __attribute__((noinline)) int probe_prune_step_call(const int64_t *lens, double *near, int n, int j, bool live,
                                                               float d, float r, int need, int ld) {
    return probe_prune_step(lens, near, n, j, live, d, r, need, ld);
}

// DOT (fp32 rows; the center ranking in front of a shadow scan): q.row is accumulated beside the exact distance over the
// same loads, and the threads that emit the k rows also write t = -2 q.row to pair_t[q * k + rank] -- the pair terms of
// the list scan that follows, in probe order, for one more accumulator instead of a kernel of 10 240 dot products.
// emit (DOT only; cnt null: off): the same threads do the plan's counting for the lists they emit (plan_count_kernel's
// work, PlanEmit in pgv_internal.h): cnt[list] += 1, and through LDS the query's probe_off prefix and seg_len.  cnt was
// cleared by the topk_kernel in front of this launch.  Fill rows (-1) count nothing and have length 0.
template <typename T, bool DOT = false>
__global__ __launch_bounds__(kQThreads) void batch_recheck_kernel(
    const char *__restrict__ vectors, const uint64_t *__restrict__ tids, int nvec, int lg,
    const char *__restrict__ queries, int kprime, int k, const float *__restrict__ approx_val,
    const int64_t *__restrict__ cand_pos, const int64_t *__restrict__ cand_slot,
    const int64_t *__restrict__ list_off, const int32_t *__restrict__ probe_lists,
    const int64_t *__restrict__ probe_off, int probes,
    const int64_t *__restrict__ seg_start, int64_t fixed_len,
    const unsigned *__restrict__ row_norm_max, ScanBound bound, const float *__restrict__ eps_add, int nq,
    float *__restrict__ out_dist, int64_t *__restrict__ out_slot, uint64_t *__restrict__ out_tid,
    int32_t *__restrict__ out_i32, int32_t *__restrict__ flags, float *__restrict__ pair_t, PlanEmit emit) {
    static_assert(!DOT || std::is_same<T, float>::value, "pair terms: fp32 rows");
    __shared__ float exact[kRecheckCap];
    __shared__ float dots[DOT ? kRecheckCap : 1];
    __shared__ __attribute__((aligned(16))) unsigned long long ent[kRecheckCap];
    const int q = blockIdx.x;
    const size_t row_bytes = (size_t)nvec * sizeof(Raw16);
    // rows the candidates were picked from (DOT: the ranking, always one dense run -- launch_exact_tail checks it -- whose
    // positions are the slots: the list plan's arguments are not looked at, and cost the instantiation no registers)
    const int64_t m = (!DOT && seg_start) ? seg_start[q + 1] - seg_start[q] : fixed_len;
    const int ncand = (int)(m < kprime ? m : (int64_t)kprime);
    const int kk = ncand < k ? ncand : k;
    // Only candidates within 2 eps of the k-th approximate value can be in the head: the k smallest-approx rows have
    // exact <= approx[k] + eps, every row with approx > approx[k] + 2 eps has exact > approx[k] + eps.  The candidates
    // come sorted (float8 order, NaN last), so the band is a prefix; it is usually k + a few of the k' rows.
    const float *av = approx_val + (size_t)q * kprime;
    // |q|^2 for the bound (the approximate values carry none: it would shift a query's values alike)
    __shared__ float qn_part[kQWaves];
    {
        const char *qrow = queries + (size_t)q * row_bytes;
        float a = 0.f;
        for (int v = threadIdx.x; v < nvec; v += kQThreads) {
            const Raw16 x = load16(qrow + (size_t)v * sizeof(Raw16));
            a = accum_slice<T, 1>(a, x, x);
        }
        for (int m2 = 32; m2 > 0; m2 >>= 1) a += __shfl_xor(a, m2);
        if ((threadIdx.x & (kWave - 1)) == 0) qn_part[threadIdx.x >> 6] = a;
    }
    __syncthreads();
    float qn = 0.f;
    for (int w = 0; w < kQWaves; w++) qn += qn_part[w];
    const float rn = __uint_as_float(*row_norm_max);
    // (pgv_internal.h, ScanBound; the norms computed here and there carry a relative error of a few u themselves:
    // one part in a thousand on top covers it)
    const float cross = 2.f * sqrtf(qn * rn);
    // (eps_add: the per-query term of the shadow scan, ScanBound)
    const float eps = 1.001f * (bound.g_sq * (qn + rn + cross) + bound.g_dot * cross + bound.g_norm * rn +
                                (eps_add ? eps_add[q] : 0.f));
    // NaN / inf anywhere: everything is in the band
    unsigned band = 0u;
    if (kk > 0) {
        const float edge = av[kk - 1] + 2.f * eps;
        band = float_to_key(edge + bound.g_ref * fabsf(edge + qn));
    }
    const int cnt = __syncthreads_count((int)threadIdx.x < ncand && float_to_key(av[threadIdx.x]) <= band);
    // the candidates' row slots: given (the center ranking: a center's position is its id), or worked out here from
    // the positions in the query's segment (the list scan; what positions_to_slots_kernel does for the exact paths)
    __shared__ int64_t slots[kRecheckCap];
    if ((int)threadIdx.x < cnt) {
        const int64_t p = cand_pos[(size_t)q * kprime + threadIdx.x];
        int64_t slot = p;
        if constexpr (DOT) {
        } else if (cand_slot) {
            slot = cand_slot[(size_t)q * kprime + threadIdx.x];
        } else {
            const int64_t *off = probe_off + (size_t)q * probes;
            int lo = 0, hi = probes - 1;  // last probe whose offset <= p
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (off[mid] <= p)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            slot = list_off[probe_lists[(size_t)q * probes + lo]] + (p - off[lo]);
        }
        slots[threadIdx.x] = slot;
    }
    __syncthreads();
    if constexpr (DOT)
        score_rows_dot([&](int64_t j) { return vectors + (size_t)slots[j] * row_bytes; }, 0, cnt,
                       queries + (size_t)q * row_bytes, nvec, lg, exact, dots);
    else
        score_rows<T, 0, 0>([&](int64_t j) { return vectors + (size_t)slots[j] * row_bytes; }, 0, cnt,
                            queries + (size_t)q * row_bytes, nvec, lg, exact);
    __syncthreads();
    if ((int)threadIdx.x < kRecheckCap)
        ent[threadIdx.x] = (int)threadIdx.x < cnt
                               ? ((unsigned long long)float_to_key(exact[threadIdx.x]) << 32) |
                                     (unsigned)cand_pos[(size_t)q * kprime + threadIdx.x]
                               : ~0ull;
    __syncthreads();
    // sort by (exact distance, position in the stream): every thread ranks its own entry
    const unsigned long long mine = ent[threadIdx.x];
    const int64_t my_slot = (int)threadIdx.x < cnt ? slots[threadIdx.x] : -1;
    int rank = 0;
    {
        const ulonglong2 *e2 = reinterpret_cast<const ulonglong2 *>(ent);
        const int n2 = (cnt + 1) / 2;
#pragma unroll 8
        for (int j = 0; j < n2; j++) {
            const ulonglong2 o = e2[j];
            rank += o.x < mine ? 1 : 0;
            rank += o.y < mine ? 1 : 0;
        }
    }
    if ((int)threadIdx.x < cnt && rank < k) {
        const size_t o = (size_t)q * k + rank;
        out_dist[o] = key_to_float((unsigned)(mine >> 32));
        if constexpr (!DOT) {
            if (out_slot) out_slot[o] = my_slot;
            if (out_tid) out_tid[o] = tids ? tids[my_slot] : ~0ull;
        }
        if (out_i32) out_i32[o] = (int32_t)my_slot;
        if constexpr (DOT) pair_t[o] = -2.f * dots[threadIdx.x];
    }
    if ((int)threadIdx.x >= kk && (int)threadIdx.x < k) {  // fewer tuples than the head asked for
        const size_t o = (size_t)q * k + threadIdx.x;
        out_dist[o] = INFINITY;
        if constexpr (!DOT) {
            if (out_slot) out_slot[o] = -1;
            if (out_tid) out_tid[o] = ~0ull;
        }
        if (out_i32) out_i32[o] = -1;
        if constexpr (DOT) pair_t[o] = 0.f;
    }
    if constexpr (DOT) {
        if (emit.cnt) {  // (block-uniform; k <= kRecheckCap)
            __syncthreads();  // every thread has read its slot and ranked itself: slots[] and ent[] are free
            const bool emits = (int)threadIdx.x < cnt && rank < k;
            const bool fills = (int)threadIdx.x >= kk && (int)threadIdx.x < k;  // (a fill entry: no rows, near side 0)
            if (emits) slots[rank] = emit.list_off[my_slot + 1] - emit.list_off[my_slot];
            if (fills) slots[threadIdx.x] = 0;
            bool drop = false;
            if (emit.radius) {  // (block-uniform) probe pruning, by the threads that emit
                const int res = probe_prune_step(slots, reinterpret_cast<double *>(ent), k,
                                                 emits ? rank : (fills ? (int)threadIdx.x : -1), emits,
                                                 key_to_float((unsigned)(mine >> 32)), emits ? emit.radius[my_slot] : 0.f,
                                                 emit.need, nvec * 4);
                drop = (res & 1) != 0;  // (every thread has read the lengths it needs: a barrier lies behind them)
                if (drop) {
                    const size_t o = (size_t)q * k + rank;
                    slots[rank] = 0;
                    out_i32[o] = -1;
                    pair_t[o] = 0.f;
                }
            }
            if (emits && !drop) atomicAdd(&emit.cnt[my_slot], 1);
            __syncthreads();
            if ((int)threadIdx.x < k) {
                int64_t run = 0;
                for (int i = 0; i < (int)threadIdx.x; i++) run += slots[i];
                emit.probe_off[(size_t)q * k + threadIdx.x] = run;
                if ((int)threadIdx.x == k - 1) emit.seg_len[q] = run + slots[threadIdx.x];
            }
        }
    }
    if (threadIdx.x == 0) {
        // the band reaches the end of the candidates and there are rows beyond them: one of those may be in it too
        const int32_t flag = (m > ncand && cnt == ncand) ? 1 : 0;
        flags[q] = flag;
        if (flag) flags[nq + 1 + atomicAdd(&flags[nq], 1)] = q;  // [nq] flags | count | list of flagged queries
    }
}

// The flagged queries, start to end in one launch (they are rare -- none on ordinary data -- so the three launches
// this used to be were three dependent kernel boundaries for nothing).  A workgroup takes a flagged query and
//   (1) WIDENS its candidate set: the kWide = 256 smallest approximate values of the segment (still in seg_vals),
//       the rounding band around the k-th of them, the exact distances of the rows in the band.  When the band ends
//       inside the 256 (or the segment has no more rows), the head is complete: sort by (exact distance, position),
//       write the query's output row.  This settles a band that was a few dozen candidates too wide for k' at ~1 %
//       of the cost of (2) (fp16 at 3072 dimensions under the deterministic bound: one query in nine).
//   (2) otherwise scores every row of its segment with the exact form (the whole segment, what the exact kernels would
//       have done), selects the head like topk_kernel and writes the query's output row.
// Workgroups without a flagged query leave at once.
// emit (with pair_t: the ranking in front of a shadow scan; cnt null: off): batch_recheck_kernel has counted the lists
// it emitted for the query; its row is replaced here, so the old lists are taken out of cnt again, the new ones added,
// and the query's probe_off and seg_len rewritten (k <= kWide).
constexpr int kWide = kRecheckCap;

template <typename T>
__global__ __launch_bounds__(kQThreads) void batch_fix_kernel(
    const char *__restrict__ vectors, const int64_t *__restrict__ list_off, const uint64_t *__restrict__ tids, int nvec,
    int lg, const char *__restrict__ queries, const int32_t *__restrict__ probe_lists,
    const int64_t *__restrict__ probe_off, int probes, const int64_t *__restrict__ seg_start, int64_t fixed_len,
    const int32_t *__restrict__ flags, int nq, float *__restrict__ seg_vals, int k, int kp, int cap,
    const unsigned *__restrict__ row_norm_max, ScanBound bound, const float *__restrict__ eps_add, int widen,
    float *__restrict__ out_dist, int64_t *__restrict__ out_slot, uint64_t *__restrict__ out_tid,
    int32_t *__restrict__ out_i32, double *__restrict__ stats, float *__restrict__ pair_t, PlanEmit emit) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long *ent = reinterpret_cast<unsigned long long *>(smem);  // [cap >= max(kp, kWide)]
    SelShared *sel = reinterpret_cast<SelShared *>(smem + (size_t)cap * 8);
    __shared__ float exact[kWide];
    __shared__ int64_t slots[kWide];
    __shared__ float qn_part[kQWaves];
    const int nflag = flags[nq];
    const size_t row_bytes = (size_t)nvec * sizeof(Raw16);
    for (int f = blockIdx.x; f < nflag; f += gridDim.x) {
        const int q = flags[nq + 1 + f];
        // probe_lists == null: the rows are one dense run (the centers), every query's segment is all of them
        const int64_t base = probe_lists ? seg_start[q] : (int64_t)q * fixed_len;
        const int64_t m = probe_lists ? seg_start[q + 1] - base : fixed_len;
        const int64_t *off = probe_off + (size_t)q * probes;
        const int32_t *pl = probe_lists + (size_t)q * probes;
        auto slot_of = [&](int64_t j) -> int64_t {  // position in the segment -> row slot
            if (!probe_lists) return j;
            int lo = 0, hi = probes - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (off[mid] <= j)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            return list_off[pl[lo]] + (j - off[lo]);
        };
        float *v = seg_vals + base;
        const char *qrow = queries + (size_t)q * row_bytes;
        // pair_t (fp32 rows; the ranking in front of a shadow scan): the pair terms of the output row this workgroup
        // writes -- batch_recheck_kernel's were those of the lists it emitted, which are being replaced
        auto pair_terms = [&]() {
            if constexpr (std::is_same<T, float>::value) {
                if (pair_t) {
                    __threadfence();
                    __syncthreads();
                    fill_pair_terms(vectors, row_bytes, qrow, nvec * 4, out_i32 ? out_i32 + (size_t)q * k : nullptr,
                                    out_slot ? out_slot + (size_t)q * k : nullptr, k, pair_t + (size_t)q * k);
                    if (emit.cnt) {  // the new row's lists into the plan (slots[] is free: a barrier lies behind its readers)
                        // (ent[] is free as well: probe_prune_step's scratch, as in batch_recheck_kernel's emit)
                        const bool mine_k = (int)threadIdx.x < k;
                        const size_t o = (size_t)q * k + threadIdx.x;
                        int l = -1;
                        if (mine_k) {
                            l = __hip_atomic_load(out_i32 + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            slots[threadIdx.x] = l >= 0 ? emit.list_off[l + 1] - emit.list_off[l] : 0;
                        }
                        if (emit.radius) {  // (block-uniform) probe pruning of the new row
                            const int res = probe_prune_step_call(
                                slots, reinterpret_cast<double *>(ent), k, mine_k ? (int)threadIdx.x : -1, l >= 0,
                                mine_k ? __hip_atomic_load(out_dist + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f,
                                l >= 0 ? emit.radius[l] : 0.f, emit.need, nvec * 4);
                            if (res & 1) {  // (every thread has read the lengths it needs: a barrier lies behind them)
                                slots[threadIdx.x] = 0;
                                out_i32[o] = -1;
                                pair_t[o] = 0.f;
                                l = -1;
                            }
                        }
                        if (mine_k && l >= 0) atomicAdd(&emit.cnt[l], 1);
                        __syncthreads();
                        if ((int)threadIdx.x < k) {
                            int64_t run = 0;
                            for (int i = 0; i < (int)threadIdx.x; i++) run += slots[i];
                            emit.probe_off[(size_t)q * k + threadIdx.x] = run;
                            if ((int)threadIdx.x == k - 1) emit.seg_len[q] = run + slots[threadIdx.x];
                        }
                    }
                }
            }
        };
        if constexpr (std::is_same<T, float>::value) {
            if (pair_t && emit.cnt) {  // (block-uniform) the lists batch_recheck_kernel emitted and counted: out again
                if ((int)threadIdx.x < k) {
                    const int l = out_i32[(size_t)q * k + threadIdx.x];
                    if (l >= 0) atomicSub(&emit.cnt[l], 1);
                }
                __syncthreads();  // read before any thread of this workgroup writes the new row
            }
        }
        bool settled = false;
        if (widen && k <= kWide / 2) {
            // (1) the kWide smallest approximate values, ascending by (value, position)
            const int nw = (int)(m < kWide ? m : (int64_t)kWide);
            block_topk([v](int64_t i) { return v[i]; }, m, nw, kWide, cap, ent, sel);
            {
                float a = 0.f;
                for (int x = threadIdx.x; x < nvec; x += kQThreads) {
                    const Raw16 e = load16(qrow + (size_t)x * sizeof(Raw16));
                    a = accum_slice<T, 1>(a, e, e);
                }
                for (int m2 = 32; m2 > 0; m2 >>= 1) a += __shfl_xor(a, m2);
                if ((threadIdx.x & (kWave - 1)) == 0) qn_part[threadIdx.x >> 6] = a;
            }
            __syncthreads();
            float qn = 0.f;
            for (int w = 0; w < kQWaves; w++) qn += qn_part[w];
            const float rn = __uint_as_float(*row_norm_max);
            const float cross = 2.f * sqrtf(qn * rn);
            const float eps = 1.001f * (bound.g_sq * (qn + rn + cross) + bound.g_dot * cross + bound.g_norm * rn +
                                        (eps_add ? eps_add[q] : 0.f));
            const int kk = nw < k ? nw : k;
            unsigned band = 0u;
            if (kk > 0) {
                const float edge = key_to_float((unsigned)(ent[kk - 1] >> 32)) + 2.f * eps;
                band = float_to_key(edge + bound.g_ref * fabsf(edge + qn));
            }
            const int cnt = __syncthreads_count((int)threadIdx.x < nw && (unsigned)(ent[threadIdx.x] >> 32) <= band);
            settled = !(m > nw && cnt == nw);  // (block-uniform)
            if (settled) {
                const unsigned my_pos = (int)threadIdx.x < cnt ? (unsigned)(ent[threadIdx.x] & 0xffffffffu) : 0u;
                if ((int)threadIdx.x < cnt) slots[threadIdx.x] = slot_of((int64_t)my_pos);
                __syncthreads();
                score_rows<T, 0, 0>([&](int64_t j) { return vectors + (size_t)slots[j] * row_bytes; }, 0, cnt, qrow, nvec, lg,
                                    exact);
                __syncthreads();
                if ((int)threadIdx.x < kWide)
                    ent[threadIdx.x] = (int)threadIdx.x < cnt
                                           ? ((unsigned long long)float_to_key(exact[threadIdx.x]) << 32) | my_pos
                                           : ~0ull;
                __syncthreads();
                const unsigned long long mine = ent[threadIdx.x];
                int rank = 0;
                for (int j = 0; j < cnt; j++) rank += ent[j] < mine ? 1 : 0;
                const int have = (int)(m < k ? m : (int64_t)k);
                if ((int)threadIdx.x < cnt && rank < k) {
                    const size_t o = (size_t)q * k + rank;
                    const int64_t slot = slots[threadIdx.x];
                    out_dist[o] = key_to_float((unsigned)(mine >> 32));
                    if (out_slot) out_slot[o] = slot;
                    if (out_i32) out_i32[o] = (int32_t)slot;
                    if (out_tid) out_tid[o] = tids ? tids[slot] : ~0ull;
                }
                if ((int)threadIdx.x >= have && (int)threadIdx.x < k) {
                    const size_t o = (size_t)q * k + threadIdx.x;
                    out_dist[o] = INFINITY;
                    if (out_slot) out_slot[o] = -1;
                    if (out_i32) out_i32[o] = -1;
                    if (out_tid) out_tid[o] = ~0ull;
                }
                if (stats && threadIdx.x == 0) atomicAdd(&stats[7], 1.0);  // profiling: settled by the wider candidate set
                pair_terms();
            }
            __syncthreads();  // ent / exact / slots are reused
        }
        if (settled) continue;
        if (stats && threadIdx.x == 0) atomicAdd(&stats[6], 1.0);  // profiling: queries that took the exact pass
        score_rows<T, 0, 0>([&](int64_t j) { return vectors + (size_t)slot_of(j) * row_bytes; }, 0, m, qrow, nvec, lg, v);
        __threadfence();
        __syncthreads();
        // the values were written by this workgroup's other wavefronts a moment ago: agent-scope loads, so that a
        // line of the vector L1 that was cached before (a neighbouring segment's selection) cannot serve them stale
        block_topk([v](int64_t i) { return __hip_atomic_load(v + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }, m, k, kp,
                   cap, ent, sel);
        for (int i = threadIdx.x; i < k; i += kQThreads) {
            const unsigned long long e = ent[i];
            const bool have = e != ~0ull && (int64_t)i < (m < k ? m : (int64_t)k);
            const int64_t slot = have ? slot_of((int64_t)(unsigned)(e & 0xffffffffu)) : -1;
            out_dist[(size_t)q * k + i] = have ? key_to_float((unsigned)(e >> 32)) : INFINITY;
            if (out_slot) out_slot[(size_t)q * k + i] = slot;
            if (out_i32) out_i32[(size_t)q * k + i] = (int32_t)slot;
            if (out_tid) out_tid[(size_t)q * k + i] = (have && tids) ? tids[slot] : ~0ull;
        }
        pair_terms();
        __syncthreads();  // ent / sel are reused by the next flagged query
    }
}

// Probe pruning for probe lists that were GIVEN (pgv_scan_batch over the row shadow; pgv_internal.h, beside ScanBound): one
// workgroup per query, in front of the plan, does for the query's lists what the ranking's recheck does for the lists it
// emits -- the exact center distances and q.c_l by the same score_rows_dot (the same bits), the rule by the same
// probe_dropped -- and leaves the lists with the dropped ones as -1 and every pair's t = -2 q.c_l (0 where there is no
// list).  A list id < 0 in the input is a fill entry: no rows, nothing to drop.  probes <= kRecheckCap
static_assert(kRecheckCap <= kQThreads, "a thread per probe");
__global__ __launch_bounds__(kQThreads) void probe_prune_kernel(
    const char *__restrict__ centers, const float *__restrict__ radius, const int64_t *__restrict__ list_off, int nvec,
    int lg, const char *__restrict__ queries, const int32_t *__restrict__ probe_lists, int probes, int need,
    int32_t *__restrict__ out_lists, float *__restrict__ pair_t) {
    __shared__ float exact[kRecheckCap], dots[kRecheckCap];
    __shared__ int64_t lens[kRecheckCap];
    __shared__ double near[kRecheckCap];
    __shared__ int32_t lists[kRecheckCap];
    const int q = blockIdx.x;
    const size_t row_bytes = (size_t)nvec * sizeof(Raw16);
    const bool mine = (int)threadIdx.x < probes;
    if (mine) lists[threadIdx.x] = probe_lists[(size_t)q * probes + threadIdx.x];
    __syncthreads();
    score_rows_dot([&](int64_t j) { return centers + (size_t)(lists[j] < 0 ? 0 : lists[j]) * row_bytes; }, 0, probes,
                   queries + (size_t)q * row_bytes, nvec, lg, exact, dots);
    __syncthreads();
    const int l = mine ? lists[threadIdx.x] : -1;
    if (mine) lens[threadIdx.x] = l >= 0 ? list_off[l + 1] - list_off[l] : 0;
    const int res = probe_prune_step(lens, near, probes, mine ? (int)threadIdx.x : -1, l >= 0, mine ? exact[threadIdx.x] : 0.f,
                                     l >= 0 ? radius[l] : 0.f, need, nvec * 4);
    const bool drop = (res & 1) != 0;
    if (mine) {
        const size_t o = (size_t)q * probes + threadIdx.x;
        out_lists[o] = drop ? -1 : l;
        pair_t[o] = (drop || l < 0) ? 0.f : -2.f * dots[threadIdx.x];
    }
}

constexpr size_t kQueryLds = (size_t)kHeadCap * 8 + sizeof(SelShared);

// rows per workgroup run and workgroups: one wavefront step per run (two rows per wavefront for
// whole-slice rows) so that every row is in flight at once; at most 8 workgroups per CU
void run_geometry(pgv_ctx *ctx, const RowGeom &g, int64_t nrows, int *per, int *grid) {
    const bool whole = g.lpr_log2 == 6 && g.nvec % kWave == 0;
    const int step = kQWaves * (whole ? 2 : (kWave >> g.lpr_log2));
    int64_t runs = (nrows + step - 1) / step;
    const int64_t cap = (int64_t)ctx->num_cus * 8;
    *per = step;
    *grid = (int)(runs < 1 ? 1 : (runs > cap ? cap : runs));
}

int pow2_at_least(int k) {
    int kp = 2;
    while (kp < k) kp <<= 1;
    return kp;
}

// whole-slice row shapes get the register-resident query; everything else the generic loop
template <typename T, int METRIC, typename F> int dispatch_nch(const RowGeom &g, F f) {
    if (g.lpr_log2 == 6 && g.nvec % kWave == 0) {
        switch (g.nvec / kWave) {
            case 1: return f(std::integral_constant<int, 1>());
            case 2: return f(std::integral_constant<int, 2>());
            case 3: return f(std::integral_constant<int, 3>());
            case 4: return f(std::integral_constant<int, 4>());
            case 6: return f(std::integral_constant<int, 6>());
        }
    }
    return f(std::integral_constant<int, 0>());
}

}  // namespace

int query_max_batch_lists() { return kMaxBatchLists; }
int query_head_cap() { return kHeadCap; }

int launch_query_stage(pgv_ctx *ctx, const void *src_pinned, void *dst_dev, int nvec) {
    hipLaunchKernelGGL(query_stage_kernel, dim3(1), dim3(1024), 0, ctx->stream, static_cast<const Raw16 *>(src_pinned),
                       static_cast<Raw16 *>(dst_dev), nvec);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_query_iota(pgv_ctx *ctx, int32_t *out, int n) {
    hipLaunchKernelGGL(query_iota_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, out, n);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

// nq queries (the rows of q_dev) against v's contiguous rows, out[q * out_stride + j] = distance of query q to row j:
// query_rank_kernel, the streaming form (whole rows in flight per wavefront, the query in registers) -- the centers of
// GetScanLists for one query or a few, a k-means++ round over the samples, pgv_distance_batch
int launch_query_rows(pgv_ctx *ctx, const RowsView &v, const void *q_dev, int nq, float *out, int64_t out_stride) {
    if (v.n <= 0 || nq <= 0) return PGV_OK;
    if (v.bits()) PGV_FAIL(PGV_ERR_ARG, "queries over rows: fp32 / fp16 rows only");
    const RowGeom &g = v.geom;
    int per, grid;
    run_geometry(ctx, g, v.n, &per, &grid);
    return dispatch_metric(v.metric, v.dtype(), [&](auto *tp, auto mc) {
        using T = std::remove_pointer_t<decltype(tp)>;
        constexpr int M = decltype(mc)::value;
        return dispatch_nch<T, M>(g, [&](auto nc) {
            constexpr int NCH = decltype(nc)::value;
            hipLaunchKernelGGL((query_rank_kernel<T, M, NCH>), dim3(grid, nq), dim3(kQThreads), 0, ctx->stream,
                               static_cast<const char *>(v.rows), (int)v.n, g.nvec, g.lpr_log2,
                               static_cast<const char *>(q_dev), out, out_stride, per);
            PGV_HIP(hipGetLastError());
            return PGV_OK;
        });
    });
}

// GetScanLists for nq staged queries: cdist[q * cd_stride + list], then the max_probes nearest of each query
int launch_query_rank(pgv_ctx *ctx, const pgv_index *ix, const void *q_dev, int nq, float *cdist, int64_t cd_stride,
                      int max_probes, int32_t *out_lists, float *out_dist) {
    PGV_TRY(launch_query_rows(ctx, ivf_centers(ix), q_dev, nq, cdist, cd_stride));
    hipLaunchKernelGGL(query_lists_kernel, dim3(nq), dim3(kQThreads), kQueryLds, ctx->stream, cdist, cd_stride, ix->nlists,
                       max_probes, pow2_at_least(max_probes), out_lists, out_dist);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

// GetScanItems for nq staged queries (q_dev null: one NULL query), query q over probe_lists[q * nprobes ..] into
// seg[q * seg_stride ..]; rows_bound: rows no query's lists exceed
int launch_query_scan(pgv_ctx *ctx, const pgv_index *ix, const void *q_dev, int nq, const int32_t *probe_lists,
                      int nprobes, int64_t rows_bound, float *seg, int64_t seg_stride) {
    const RowGeom &g = ix->geom;
    int per, grid;
    run_geometry(ctx, g, rows_bound, &per, &grid);
    // nq grid rows share the device: a row needs no more workgroups than keep every CU busy (one row: run_geometry's cap)
    const int cap = (ctx->num_cus * 8 + nq - 1) / nq;
    if (grid > cap) grid = cap < 1 ? 1 : cap;
    return dispatch_metric(ix->metric, ix->dtype, [&](auto *tp, auto mc) {
        using T = std::remove_pointer_t<decltype(tp)>;
        constexpr int M = decltype(mc)::value;
        return dispatch_nch<T, M>(g, [&](auto nc) {
            constexpr int NCH = decltype(nc)::value;
            hipLaunchKernelGGL((query_scan_kernel<T, M, NCH>), dim3(grid, nq), dim3(kQThreads), 0, ctx->stream,
                               static_cast<const char *>(ix->vectors), ix->list_offsets, probe_lists, nprobes, g.nvec,
                               g.lpr_log2, static_cast<const char *>(q_dev), seg, seg_stride, per);
            PGV_HIP(hipGetLastError());
            return PGV_OK;
        });
    });
}

int launch_query_head(pgv_ctx *ctx, const pgv_index *ix, const float *seg, const int32_t *probe_lists, int nprobes,
                      int skip, int count, void *head_rec, unsigned seq) {
    hipLaunchKernelGGL(query_head_kernel, dim3(1), dim3(kQThreads), kQueryLds, ctx->stream, seg, ix->list_offsets,
                       ix->tids, probe_lists, nprobes, skip, count, pow2_at_least(skip + count),
                       static_cast<QueryHead *>(head_rec), query_head_dists(head_rec, count), query_head_slots(head_rec),
                       query_head_tids(head_rec, count), seq);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

// a few queries at a time: the head of every query's sorted stream into the caller's [nq x k] device arrays
int launch_multi_head(pgv_ctx *ctx, const pgv_index *ix, int nq, const float *seg, int64_t seg_stride,
                      const int32_t *probe_lists, int nprobes, int k, float *out_dist, int64_t *out_slot,
                      uint64_t *out_tid) {
    double *stats = (ctx->profiling && ctx->stats_dev.p) ? ctx->stats_dev.as<double>() : nullptr;
    hipLaunchKernelGGL(mq_head_kernel, dim3(nq), dim3(kQThreads), kQueryLds, ctx->stream, seg, seg_stride, ix->list_offsets,
                       ix->tids, probe_lists, nprobes, k, pow2_at_least(k), out_dist, out_slot, out_tid, stats);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int probe_prune_max_probes() { return kRecheckCap; }

int launch_probe_prune(pgv_ctx *ctx, const pgv_index *ix, const void *q_dev, int nq, const int32_t *probe_lists, int probes,
                       int need, int32_t *out_lists, float *pair_t) {
    if (nq <= 0) return PGV_OK;
    if (probes < 1 || probes > kRecheckCap || !ix->list_radius || ix->dtype != PGV_F32)
        PGV_FAIL(PGV_ERR_ARG, "probe pruning: fp32 rows with list radii, 1..%d probes", kRecheckCap);
    hipLaunchKernelGGL(probe_prune_kernel, dim3(nq), dim3(kQThreads), 0, ctx->stream, static_cast<const char *>(ix->centers),
                       ix->list_radius, ix->list_offsets, ix->geom.nvec, ix->geom.lpr_log2, static_cast<const char *>(q_dev),
                       probe_lists, probes, need, out_lists, pair_t);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

namespace {
struct ApproxScratch {  // the tail's candidates and flags, carved from the caller's buffer
    float *cand_val = nullptr;   // [nq x kprime] approximate values, ascending
    int64_t *cand_pos = nullptr; // [nq x kprime] positions in the query's segment (the row slots of a dense run)
    int32_t *flags = nullptr;    // [nq] flags | count | list of flagged queries
    int carve(DBuf &buf, int nq, int kprime) {
        const size_t nk = (size_t)nq * kprime;
        const size_t a1 = (sizeof(float) * nk + 15) & ~(size_t)15, a2 = a1 + sizeof(int64_t) * nk;
        PGV_TRY(buf.ensure(a2 + sizeof(int32_t) * (2 * (size_t)nq + 1)));
        cand_val = buf.as<float>();
        cand_pos = reinterpret_cast<int64_t *>(buf.as<char>() + a1);
        flags = reinterpret_cast<int32_t *>(buf.as<char>() + a2);
        return PGV_OK;
    }
};
}  // namespace

int launch_exact_tail(pgv_ctx *ctx, const ExactTail &t, DBuf &scratch) {
    if (t.nq <= 0) return PGV_OK;
    const ExactRows &xr = t.rows;
    const bool dense = t.dense();
    if (dense ? (t.fixed_len <= 0 || t.probe_off || t.seg_start || t.probes != 0)
              : (t.fixed_len != 0 || !t.probe_off || !t.seg_start || t.probes < 1))
        PGV_FAIL(PGV_ERR_ARG, "exact tail: a list plan or one dense run");
    if (t.kprime > kRecheckCap || t.k > t.kprime)
        PGV_FAIL(PGV_ERR_ARG, "exact tail: k' = %d outside k..%d", t.kprime, kRecheckCap);
    if (t.pair_t && (xr.dtype != PGV_F32 || !dense || t.out_slot || t.out_tid || !t.out_i32))
        PGV_FAIL(PGV_ERR_ARG, "exact tail: pair terms are for one dense run of fp32 rows whose slots leave as int32");
    static_assert(kWide >= kRecheckCap, "k <= k' <= kWide: batch_fix_kernel's emit");
    if (t.emit.cnt && !(dense && t.pair_t && t.out_i32 && t.emit.probe_off && t.emit.seg_len && t.emit.list_off))
        PGV_FAIL(PGV_ERR_ARG, "exact tail: the plan is counted where the pair terms are written");
    ApproxScratch sc;
    PGV_TRY(sc.carve(scratch, t.nq, t.kprime));
    const int64_t *cand_slot = dense ? sc.cand_pos : nullptr;  // a dense run's positions ARE the slots
    const int64_t *seg_start = dense ? nullptr : t.seg_start;
    const int64_t fixed_len = dense ? t.fixed_len : 0;
    // flags[nq], the flagged-query count, starts from zero; so do the plan's cnt | fill under emit (one word per list
    // each; the ranking's rows are the centers: fixed_len lists)
    PGV_TRY(launch_topk_segments(ctx, t.approx, seg_start, t.nq, fixed_len, t.kprime, sc.cand_val, sc.cand_pos,
                                 sc.flags + t.nq, t.emit.cnt, t.emit.cnt ? 2 * (int)fixed_len : 0,
                                 dense ? 0 : t.seg_bound));
#define PGV_RECHECK(T, DOT)                                                                                          \
    hipLaunchKernelGGL((batch_recheck_kernel<T, DOT>), dim3(t.nq), dim3(kQThreads), 0, ctx->stream,                   \
                       static_cast<const char *>(xr.vectors), xr.tids, xr.geom.nvec, xr.geom.lpr_log2,                \
                       static_cast<const char *>(t.queries), t.kprime, t.k, sc.cand_val, sc.cand_pos, cand_slot,      \
                       xr.list_offsets, t.probe_lists, t.probe_off, t.probes, seg_start, fixed_len, xr.norm_max,      \
                       t.bound, t.eps_add, t.nq, t.out_dist, t.out_slot, t.out_tid, t.out_i32, sc.flags, t.pair_t,    \
                       t.emit)
    if (t.pair_t)
        PGV_RECHECK(float, true);
    else if (xr.dtype == PGV_F32)
        PGV_RECHECK(float, false);
    else
        PGV_RECHECK(__half, false);
#undef PGV_RECHECK
    PGV_HIP(hipGetLastError());
    // (the ranking's flagged queries count like the list scan's: pgv_stats scan_widened_queries / scan_redo_queries)
    double *stats = (ctx->profiling && ctx->stats_dev.p) ? ctx->stats_dev.as<double>() : nullptr;
    int kp = 2;
    while (kp < t.k) kp <<= 1;
    const int cap = kp > kFastCap ? kp : kFastCap;
    const size_t lds = (size_t)cap * 8 + sizeof(SelShared);
    const int grid = t.nq < ctx->num_cus ? t.nq : ctx->num_cus;
#define PGV_FIX(T)                                                                                                    \
    hipLaunchKernelGGL(batch_fix_kernel<T>, dim3(grid), dim3(kQThreads), lds, ctx->stream,                            \
                       static_cast<const char *>(xr.vectors), xr.list_offsets, xr.tids, xr.geom.nvec,                 \
                       xr.geom.lpr_log2, static_cast<const char *>(t.queries), t.probe_lists, t.probe_off, t.probes,  \
                       seg_start, fixed_len, sc.flags, t.nq, t.approx, t.k, kp, cap, xr.norm_max, t.bound, t.eps_add, \
                       ctx->no_widen ? 0 : 1, t.out_dist, t.out_slot, t.out_tid, t.out_i32, stats, t.pair_t, t.emit)
    if (xr.dtype == PGV_F32)
        PGV_FIX(float);
    else
        PGV_FIX(__half);
#undef PGV_FIX
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

}  // namespace pgv
