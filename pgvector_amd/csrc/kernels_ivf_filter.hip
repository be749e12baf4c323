// kernels_ivf_filter.hip -- the IVFFlat iterative scan under a filter (pgv_search_filtered), gfx950.
//
// The reference answers `ORDER BY emb <-> $1 LIMIT k` under a WHERE clause with ivfflat.iterative_scan = relaxed_order
// (src/ivfscan.c:134, :268-277, :400-406): scan `probes` lists, sort, let the executor drop what fails the filter, and
// scan the next `probes` lists while LIMIT is not met.  Here the filter is known before a row is touched -- a bitmap
// over row slots -- so the chain reads the bitmap first and the rows of the kept slots only:
//
//   ivf_keep_count_kernel      popcount of the keep bits of every (query, ranked list); one wavefront an item, the
//                              list's first and last words masked.  Reads the bitmap and nothing else
//   ivf_filter_plan_kernel     one workgroup a query: prefix sum of the kept counts in probe order, the last round
//                              R_q that is needed (the first whose cumulative count reaches k), out_probes /
//                              out_count / padding, one segment per round <= R_q and the score tasks of the lists
//                              of those rounds that keep anything.  A query's kept rows lie side by side in probe
//                              order, so a round's segment is a slice of that run: [pre[r probes], pre[(r + 1) probes])
//   ivf_filtered_scan_kernel   persistent workgroups pull tasks (query, row range of one list): the query into LDS, the
//                              range's kept row offsets compacted into LDS in slot order by one wavefront (a keep word a
//                              lane, popcount prefix), then ONLY the kept rows scored, by lane_rows.h's rule as
//                              scan_kernel streams them.  Value and slot land at the row's position inside its segment
//   ivf_filter_emit_kernel     pgv_select.h's selection over each segment for the rows the round can still emit
//                              (min(kept, k - emitted before)), written straight behind the earlier rounds' rows
#include "lane_rows.h"
#include "pgv_select.h"

namespace pgv {

namespace {

constexpr int kFiltThreads = 256;
constexpr int kFiltWaves = kFiltThreads / kWave;
// rows in flight per lane: scan_kernel's 8 for one query a task; 4 over fp16 rows (8 spilled 32 bytes a lane there)
template <typename T> constexpr int kFiltR = std::is_same_v<T, float> ? 8 : 4;
// rows of a task at most: their keep words (62 whole ones and a ragged one at either end) are a word a lane of ONE wavefront
constexpr int kFiltMaxTaskRows = 1984;

// word w of a bitmap with the bits outside slots [beg, end) cleared; beg >> 5 <= w <= (end - 1) >> 5
__device__ __forceinline__ uint32_t keep_word(const uint32_t *__restrict__ keep, int64_t w, int64_t beg, int64_t end) {
    uint32_t v = keep[w];
    const int64_t lo = w << 5;
    if (beg > lo) v &= ~0u << (int)(beg - lo);
    if (end < lo + 32) v &= ~0u >> (int)(lo + 32 - end);
    return v;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// item i: list i of ONE bitmap (lists == null: the counts depend on the list only), or ranked list lists[i] of query i / P
// under that query's bitmap
__global__ __launch_bounds__(kFiltThreads) void ivf_keep_count_kernel(
    const uint32_t *__restrict__ keep, int64_t keep_stride, const int32_t *__restrict__ lists, int P,
    const int64_t *__restrict__ list_off, int64_t nitems, uint32_t *__restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t item = (int64_t)blockIdx.x * kFiltWaves + (threadIdx.x >> 6);
    if (item >= nitems) return;
    const int l = lists ? lists[item] : (int)item;
    const uint32_t *bm = lists ? keep + (size_t)(item / P) * keep_stride : keep;
    unsigned c = 0;
    if (l >= 0) {
        const int64_t beg = list_off[l], end = list_off[l + 1];
        if (end > beg)
            for (int64_t w = (beg >> 5) + lane; w <= ((end - 1) >> 5); w += kWave) c += __popc(keep_word(bm, w, beg, end));
    }
    c = wave_sum_u32(c);
    if (lane == 0) out[item] = c;
}

// cnt_mode 0: no bitmap, a list keeps all its rows | 1: cnt[list] | 2: cnt[q * P + j]
__global__ __launch_bounds__(kFiltThreads) void ivf_filter_plan_kernel(
    const int32_t *__restrict__ lists, const int64_t *__restrict__ list_off, const uint32_t *__restrict__ cnt, int cnt_mode,
    int P, int probes, int k, int task_rows, int task_rows_max, unsigned long long *pre_all, unsigned long long *totals,
    IvfFilterTask *__restrict__ tasks, IvfFilterSeg *__restrict__ segs, float *__restrict__ out_dist,
    int64_t *__restrict__ out_slot, uint64_t *__restrict__ out_tid, int32_t *__restrict__ out_count,
    int32_t *__restrict__ out_probes) {
    __shared__ unsigned long long s_scan[kFiltThreads];
    __shared__ unsigned long long s_qbase;
    __shared__ int s_last;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int32_t *ql = lists + (size_t)q * P;
    unsigned long long *pre = pre_all + (size_t)q * (P + 1);  // [P + 1] kept rows in front of each ranked list; [P]: all

    unsigned long long carry = 0;
    for (int base = 0; base < P; base += kFiltThreads) {
        const int j = base + tid;
        unsigned long long c = 0;
        if (j < P) {
            const int l = ql[j];
            if (l >= 0) c = cnt_mode == 0 ? (unsigned long long)(list_off[l + 1] - list_off[l]) : cnt[cnt_mode == 1 ? (size_t)l : (size_t)q * P + j];
        }
        s_scan[tid] = c;
        __syncthreads();
        for (int st = 1; st < kFiltThreads; st <<= 1) {
            const unsigned long long t = tid >= st ? s_scan[tid - st] : 0;
            __syncthreads();
            s_scan[tid] += t;
            __syncthreads();
        }
        if (j < P) pre[j] = carry + s_scan[tid] - c;
        carry += s_scan[kFiltThreads - 1];
        __syncthreads();
    }
    const int nrounds = (P + probes - 1) / probes;
    if (tid == 0) {
        pre[P] = carry;
        s_last = nrounds - 1;
    }
    __syncthreads();  // (pre is read back below by other threads of this workgroup)

    // the stop rule: the first round whose sorted batch brings the count to k ends the scan -- reaching exactly k too
    auto round_end = [&](int r) { return (r + 1) * probes < P ? (r + 1) * probes : P; };
    for (int r = tid; r < nrounds; r += kFiltThreads)
        if (pre[round_end(r)] >= (unsigned long long)k) atomicMin(&s_last, r);
    __syncthreads();
    const int last = s_last, used = round_end(last);
    const unsigned long long total = pre[used];
    if (tid == 0) s_qbase = atomicAdd(totals, total);
    __syncthreads();
    const unsigned long long qbase = s_qbase;
    const int count = total < (unsigned long long)k ? (int)total : k;
    if (tid == 0) {
        out_count[q] = count;
        if (out_probes) out_probes[q] = used;
    }
    for (int i = count + tid; i < k; i += kFiltThreads) {
        out_dist[(size_t)q * k + i] = INFINITY;
        out_slot[(size_t)q * k + i] = -1;
        if (out_tid) out_tid[(size_t)q * k + i] = ~0ull;
    }
    // a round in front of `last` ended below k, so every round <= last still has rows to emit: k - a > 0
    for (int r = tid; r <= last; r += kFiltThreads) {
        const unsigned long long a = pre[r * probes], len = pre[round_end(r)] - a;
        if (len == 0) continue;
        const unsigned long long room = (unsigned long long)k - a;
        IvfFilterSeg s;
        s.start = (int64_t)(qbase + a);
        s.len = (uint32_t)len;
        s.query = q;
        s.kseg = (int32_t)(len < room ? len : room);
        s.out_at = (int32_t)a;
        segs[atomicAdd(totals + 2, 1ull)] = s;
    }
    // a list that keeps nothing gets no task: its rows are never read.  A selective filter gets longer row ranges (up to
    // task_rows_max) so that a task still has a wavefront's worth of kept rows; never shorter than task_rows (the bound
    // the host sized `tasks` by)
    for (int j = tid; j < used; j += kFiltThreads) {
        const unsigned long long c = pre[j + 1] - pre[j];
        if (c == 0) continue;
        const int l = ql[j];
        const int64_t beg = list_off[l], len = list_off[l + 1] - beg;
        int64_t T = ((int64_t)task_rows * len / (int64_t)c + 31) & ~(int64_t)31;
        T = T > task_rows_max ? task_rows_max : (T < task_rows ? task_rows : T);
        const int64_t nt = (len + T - 1) / T;
        const unsigned long long t0 = atomicAdd(totals + 1, (unsigned long long)nt);
        for (int64_t i = 0; i < nt; i++) {
            IvfFilterTask t;
            t.row0 = beg + i * T;
            t.out0 = (int64_t)(qbase + pre[j]);
            t.list_beg = beg;
            t.nrows = (int32_t)(len - i * T < T ? len - i * T : T);
            t.query = q;
            tasks[t0 + i] = t;
        }
    }
}

template <typename T, int METRIC>
__global__ __launch_bounds__(kFiltThreads, 4) void ivf_filtered_scan_kernel(
    const char *__restrict__ rows, const char *__restrict__ queries, const uint32_t *__restrict__ keep, int64_t keep_stride,
    const IvfFilterTask *__restrict__ tasks, const unsigned long long *__restrict__ totals, int *__restrict__ task_counter,
    float *__restrict__ out_val, int64_t *__restrict__ out_slot, int nvec, int lpr_log2, int nchunks, int kept_cap) {
    constexpr int R = kFiltR<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // layout: [nvec] Raw16 query slices | [kept_cap] uint16 kept row offsets | task id, kept rows, kept in front per wave
    Raw16 *lds_q = reinterpret_cast<Raw16 *>(smem);
    uint16_t *lds_kept = reinterpret_cast<uint16_t *>(smem + (size_t)nvec * sizeof(Raw16));
    int *lds_task = reinterpret_cast<int *>(smem + (size_t)nvec * sizeof(Raw16) + (size_t)kept_cap * sizeof(uint16_t));
    int *lds_nk = lds_task + 1;
    unsigned *lds_front = reinterpret_cast<unsigned *>(lds_task + 2);  // [kFiltWaves]

    const LaneSplit ls(lpr_log2);
    const int lane = ls.lane, wave = ls.wave;
    const size_t row_bytes = (size_t)nvec * sizeof(Raw16);
    const int ntasks = (int)totals[1];

    for (int t; pull_task(task_counter, ntasks, lds_task, &t);) {
        const IvfFilterTask task = tasks[t];
        for (int i = threadIdx.x; i < nvec; i += kFiltThreads)
            lds_q[i] = load16(queries + (size_t)task.query * row_bytes + (size_t)i * sizeof(Raw16));

        // the kept rows of [row0, row0 + nrows) as offsets from row0, in slot order, and how many the list keeps in front
        // of row0 (where this task's first value goes inside the list's run)
        if (keep) {
            const uint32_t *bm = keep + (size_t)task.query * keep_stride;
            const int64_t end = task.row0 + task.nrows;
            unsigned c = 0;
            if (task.row0 > task.list_beg)
                for (int64_t w = (task.list_beg >> 5) + threadIdx.x; w <= ((task.row0 - 1) >> 5); w += kFiltThreads)
                    c += __popc(keep_word(bm, w, task.list_beg, task.row0));
            c = wave_sum_u32(c);
            if (lane == 0) lds_front[wave] = c;
            if (wave == 0) {
                const int64_t w0 = task.row0 >> 5;
                const int nw = (int)(((end - 1) >> 5) - w0) + 1;  // <= 64: nrows <= kFiltMaxTaskRows
                uint32_t v = lane < nw ? keep_word(bm, w0 + lane, task.row0, end) : 0u;
                const int pc = __popc(v);
                int incl = pc;
#pragma unroll
                for (int s = 1; s < kWave; s <<= 1) {
                    const int o = __shfl_up(incl, s);
                    if (lane >= s) incl += o;
                }
                int at = incl - pc;
                const int off = (int)(((w0 + lane) << 5) - task.row0);  // (negative for a ragged first word: its kept bits are not)
                while (v) {
                    lds_kept[at++] = (uint16_t)(off + __ffs(v) - 1);
                    v &= v - 1;
                }
                if (lane == kWave - 1) *lds_nk = incl;
            }
        } else if (threadIdx.x == 0) {
            *lds_nk = task.nrows;
        }
        __syncthreads();
        const int nk = *lds_nk;
        int64_t front = task.row0 - task.list_beg;
        if (keep) front = (int64_t)lds_front[0] + lds_front[1] + lds_front[2] + lds_front[3];
        const int64_t out0 = task.out0 + front;
        const char *task_rows = rows + (size_t)task.row0 * row_bytes;
        auto row_of = [&](int idx) { return keep ? (int)lds_kept[idx] : idx; };

        for (int b = wave; b * R * ls.rpw < nk; b += kFiltWaves) {
            PairAcc<T, METRIC> acc[R][1];
            const char *rp[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                int idx = b * R * ls.rpw + r * ls.rpw + ls.rsub;
                idx = idx < nk ? idx : nk - 1;  // tail rows are computed, not stored
                rp[r] = task_rows + (size_t)row_of(idx) * row_bytes;
            }
            stream_rows(acc, rp, lds_q, ls, nvec, lpr_log2, nchunks);
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int idx = b * R * ls.rpw + r * ls.rpw + ls.rsub;
                acc[r][0].fold(lpr_log2);
                if (ls.last() && idx < nk) {
                    out_val[out0 + idx] = acc[r][0].value();
                    out_slot[out0 + idx] = task.row0 + row_of(idx);
                }
            }
        }
        __syncthreads();  // LDS is rewritten by the next task
    }
}

// the head of each (query, round) segment: ascending by (value in float8 order, position), ties to the lower position
// (block_topk), for as many rows as the round can still emit; the values leave as the score kernel wrote them
__global__ __launch_bounds__(kSelThreads) void ivf_filter_emit_kernel(
    const float *__restrict__ vals, const int64_t *__restrict__ slots, const IvfFilterSeg *__restrict__ segs,
    const unsigned long long *__restrict__ totals, const uint64_t *__restrict__ tids, int k, int cap,
    float *__restrict__ out_dist, int64_t *__restrict__ out_slot, uint64_t *__restrict__ out_tid) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long *ent = reinterpret_cast<unsigned long long *>(smem);  // [cap]
    SelShared *sh = reinterpret_cast<SelShared *>(smem + (size_t)cap * 8);
    const unsigned long long nseg = totals[2];
    for (unsigned long long si = blockIdx.x; si < nseg; si += gridDim.x) {
        const IvfFilterSeg seg = segs[si];
        int kp = 2;
        while (kp < seg.kseg) kp <<= 1;
        const float *v = vals + seg.start;
        block_topk_auto(v, (int64_t)seg.len, seg.kseg, kp, cap, ent, sh);
        __syncthreads();
        for (int i = threadIdx.x; i < seg.kseg; i += kSelThreads) {
            const unsigned pos = (unsigned)(ent[i] & 0xffffffffu);
            const size_t o = (size_t)seg.query * k + seg.out_at + i;
            const int64_t slot = slots[seg.start + pos];
            out_dist[o] = v[pos];
            out_slot[o] = slot;
            if (out_tid) out_tid[o] = tids[slot];
        }
        __syncthreads();  // ent is rewritten by the next segment
    }
}

}  // namespace

// PGV_IVF_FILTER_TASK_ROWS: rows of a score task, fixed (32 .. 1984, a multiple of 32); unset: 256, and up to 1984 where the
// filter keeps few of a list's rows.  Read at every call: tests split a short list over several tasks with it
void ivf_filter_task_rows(int *task_rows, int *task_rows_max) {
    const char *e = getenv("PGV_IVF_FILTER_TASK_ROWS");
    int fixed = e ? atoi(e) / 32 * 32 : 0;
    if (fixed > kFiltMaxTaskRows) fixed = kFiltMaxTaskRows;
    *task_rows = fixed >= 32 ? fixed : 256;
    *task_rows_max = fixed >= 32 ? fixed : kFiltMaxTaskRows;
}

int launch_ivf_keep_count(pgv_ctx *ctx, const uint32_t *keep, int64_t keep_stride, const int32_t *lists, int P,
                          const int64_t *list_off, int64_t nitems, uint32_t *out) {
    if (nitems <= 0) return PGV_OK;
    hipLaunchKernelGGL(ivf_keep_count_kernel, dim3((unsigned)((nitems + kFiltWaves - 1) / kFiltWaves)), dim3(kFiltThreads), 0,
                       ctx->stream, keep, keep_stride, lists, P, list_off, nitems, out);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_ivf_filter_plan(pgv_ctx *ctx, const IvfFilterPlan &p) {
    if (p.nq <= 0) return PGV_OK;
    hipLaunchKernelGGL(ivf_filter_plan_kernel, dim3(p.nq), dim3(kFiltThreads), 0, ctx->stream, p.lists, p.list_off, p.cnt,
                       p.cnt_mode, p.P, p.probes, p.k, p.task_rows, p.task_rows_max, p.pre, p.totals, p.tasks, p.segs,
                       p.out_dist, p.out_slot, p.out_tid, p.out_count, p.out_probes);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

namespace {
template <typename T, int METRIC>
int launch_filtered_scan_t(pgv_ctx *ctx, const RowsView &v, const void *queries, const uint32_t *keep, int64_t keep_stride,
                           const IvfFilterPlan &p, int64_t ntasks, float *out_val, int64_t *out_slot) {
    PGV_TRY(ctx->counters.ensure(256));
    if (!ctx->counters_clean) {
        PGV_HIP(hipMemsetAsync(ctx->counters.p, 0, 256, ctx->stream));
        ctx->counters_clean = true;
    }
    int *counter = ctx->counters.as<int>() + 12;  // words 12, 13: claimed tasks, workgroups done (the kernel re-zeroes them)
    const int kept_cap = (p.task_rows_max + 7) & ~7;
    const size_t lds = (size_t)v.geom.nvec * sizeof(Raw16) + (size_t)kept_cap * sizeof(uint16_t) + 32;
    int per_cu = (int)(160 * 1024 / (lds + 256));
    if (per_cu > 2048 / kFiltThreads) per_cu = 2048 / kFiltThreads;
    if (per_cu < 1) per_cu = 1;
    int64_t grid = (int64_t)ctx->num_cus * per_cu;
    if (grid > ntasks) grid = ntasks;
    auto kern = ivf_filtered_scan_kernel<T, METRIC>;
    if (lds > 64 * 1024)
        PGV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kFiltThreads), lds, ctx->stream, static_cast<const char *>(v.rows),
                       static_cast<const char *>(queries), keep, keep_stride, p.tasks, p.totals, counter, out_val, out_slot,
                       v.geom.nvec, v.geom.lpr_log2, v.geom.nchunks, kept_cap);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}
}  // namespace

int launch_ivf_filtered_scan(pgv_ctx *ctx, const RowsView &v, const void *queries, const uint32_t *keep, int64_t keep_stride,
                             const IvfFilterPlan &p, int64_t ntasks, float *out_val, int64_t *out_slot) {
    if (ntasks <= 0) return PGV_OK;
    if (v.bits() || v.sparse() || v.metric == PGV_L1) PGV_FAIL(PGV_ERR_ARG, "filtered scan: fp32 / fp16 rows under L2 or inner product only");
    if (ntasks > 0x7fffffff) PGV_FAIL(PGV_ERR_ARG, "filtered scan: too many tasks");
    return dispatch_metric(v.metric, v.dtype(), [&](auto *tp, auto mc) -> int {
        if constexpr (decltype(mc)::value == 2) {
            return PGV_ERR_ARG;
        } else {
            return launch_filtered_scan_t<std::remove_pointer_t<decltype(tp)>, decltype(mc)::value>(ctx, v, queries, keep, keep_stride,
                                                                                                     p, ntasks, out_val, out_slot);
        }
    });
}

int launch_ivf_filter_emit(pgv_ctx *ctx, const float *vals, const int64_t *slots, const IvfFilterPlan &p, int64_t nsegs,
                           const uint64_t *tids) {
    if (nsegs <= 0) return PGV_OK;
    int kp = 2;
    while (kp < p.k) kp <<= 1;
    const int cap = kp > kFastCap ? kp : kFastCap;
    const size_t lds = (size_t)cap * 8 + sizeof(SelShared);
    int64_t grid = (int64_t)ctx->num_cus * 8;
    if (grid > nsegs) grid = nsegs;
    hipLaunchKernelGGL(ivf_filter_emit_kernel, dim3((unsigned)grid), dim3(kSelThreads), lds, ctx->stream, vals, slots, p.segs,
                       p.totals, tids, p.k, cap, p.out_dist, p.out_slot, p.out_tid);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

}  // namespace pgv
