// lane_rows.h -- the lane-group row scorer: the one rule by which the vector ALUs compute an exact distance (device only).
//
//   * `1 << lpr_log2` adjacent lanes of a wavefront own one row (row_geom picks the power of two that wastes the fewest
//     lane-trips); each lane takes one 16-byte slice of it per trip, `rpw` rows a wavefront trip (LaneSplit).
//   * A load is never predicated: a branch around a load makes hipcc drain vmcnt per load.  A lane past the end of the row
//     clamps its address to the last slice and has its operands zeroed (`ok`), which adds nothing to any metric.
//   * R independent rows' loads are in flight per lane.  A list scan streams (stream_rows); an HNSW walk is a chain of
//     ~100 small batches, each waiting for its rows, and with one row per trip a batch of 32 neighbours was eight dependent
//     round trips to HBM per wavefront (clamped_trip; kernels_hnsw.hip score_rows).
//   * Each (row, operand) pair has ONE accumulator that takes the elements in row order (PairAcc), whatever R, QT or the
//     caller: fp32 for dense rows (fp16 converted exactly, src/halfutils.c:46-78), an integer count of differing bits for
//     bit rows (hamming_distance, src/bitvec.c:45-56) and under bit_jaccard_ops (<BitRow, 1>) a second one of the bits set
//     in either row (jaccard_distance, src/bitvec.c:60-70 over src/bitutils.c:99-131).  A bit count (<= 64 000) and every
//     partial sum of its reduction are exact in fp32, so the counts ride the same cross-lane sum.
//   * group_sum_to_last folds the lanes of a group (fold: every lane calls it), and the group's LAST lane holds the value
//     (finish<METRIC>, jaccard_value) or the walk's ordered key (float_to_key, jaccard_key).
//
// So a (row, query) pair has the same bits from pgv_scan_lists, pgv_search_filtered, pgv_hnsw_score(_pairs / _groups), the
// HNSW walk and the repair search: tests/test_gpu_lane_rows.py.  Not here, on purpose: kernels_query.hip's group_distance
// (two accumulators a lane, its own error model in pgv_internal.h), the tile and matrix-core kernels, sparse_pair.h.
#pragma once

#include <type_traits>

#include "pgv_device.h"

namespace pgv {

struct LaneSplit {
    int lane, wave;  // (a kernel that wants `wave` in a scalar register takes readfirstlane of it itself)
    int lpr;         // lanes per row
    int sub, rsub;   // which slice of the row; which row of the wave-load
    int rpw;         // rows per wave-load
    __device__ __forceinline__ explicit LaneSplit(int lpr_log2)
        : lane(threadIdx.x & (kWave - 1)), wave(threadIdx.x >> 6), lpr(1 << lpr_log2), sub(lane & (lpr - 1)),
          rsub(lane >> lpr_log2), rpw(kWave >> lpr_log2) {}
    __device__ __forceinline__ bool last() const { return sub == lpr - 1; }  // the lane a folded sum lands in
};

// one pair's accumulator.  add: a slice of either operand; MASKED && !ok: the slice is past the row's end
template <typename T, int METRIC> struct PairAcc {
    float s = 0.f;
    template <bool MASKED = true> __device__ __forceinline__ void add(const Raw16 &a, const Raw16 &b, bool ok) {
        Unpacked<T> ua(a), ub(b);
#pragma unroll
        for (int e = 0; e < VecTraits<T>::N; e++)
            s = accum<METRIC>(s, (MASKED && !ok) ? 0.f : ua.v[e], (MASKED && !ok) ? 0.f : ub.v[e]);
    }
    __device__ __forceinline__ void fold(int lpr_log2) { s = group_sum_to_last(s, lpr_log2); }
    __device__ __forceinline__ float value() const { return finish<METRIC>(s); }
    __device__ __forceinline__ uint32_t key() const { return float_to_key(value()); }
};
template <> struct PairAcc<BitRow, 0> {
    int x = 0;
    float fx;
    template <bool MASKED = true> __device__ __forceinline__ void add(const Raw16 &a, const Raw16 &b, bool ok) {
        x += (MASKED && !ok) ? 0 : hamming16(a, b);
    }
    __device__ __forceinline__ void fold(int lpr_log2) { fx = group_sum_to_last((float)x, lpr_log2); }
    __device__ __forceinline__ float value() const { return fx; }
    __device__ __forceinline__ uint32_t key() const { return float_to_key(fx); }
};
// jaccard_key orders and ties exactly as the reference's float8 does (pgv_device.h) but does not carry (x, u): a walk that
// hands distances back scores those rows once more for value()
template <> struct PairAcc<BitRow, 1> {
    int x = 0, u = 0;
    float fx, fu;
    template <bool MASKED = true> __device__ __forceinline__ void add(const Raw16 &a, const Raw16 &b, bool ok) {
        x += (MASKED && !ok) ? 0 : hamming16(a, b);
        u += (MASKED && !ok) ? 0 : union16(a, b);
    }
    __device__ __forceinline__ void fold(int lpr_log2) {
        fx = group_sum_to_last((float)x, lpr_log2);
        fu = group_sum_to_last((float)u, lpr_log2);
    }
    __device__ __forceinline__ float value() const { return jaccard_value((int)fx, (int)fu); }
    __device__ __forceinline__ uint32_t key() const { return jaccard_key((int)fx, (int)fu); }
};

// Trip c of R rows against one operand each: query(r, v) is slice v of row r's operand (gather: a row of global memory).
// The caller owns the loop over c.  The HNSW walk's score_rows and the repair search's score_batch are this trip with the
// query in LDS, written out in their kernels: through this function the fp32 walk measured 12-13 % and the fp16 repair search
// 12 % slower (profiles/r33_lane_rows.md), so they keep their copies, and tests/test_gpu_lane_rows.py holds them to the rule
template <typename T, int METRIC, int R, typename Q>
__device__ __forceinline__ void clamped_trip(PairAcc<T, METRIC> (&acc)[R], const char *const (&rp)[R], Q query,
                                             const LaneSplit &ls, int nvec, int c) {
    const int vi = c * ls.lpr + ls.sub;
    const bool ok = vi < nvec;
    const int vc = ok ? vi : nvec - 1;
    Raw16 rv[R], qv[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        rv[r] = load16(rp[r] + (size_t)vc * sizeof(Raw16));
        qv[r] = query(r, vc);
    }
#pragma unroll
    for (int r = 0; r < R; r++) acc[r].add(rv[r], qv[r], ok);
}

// R rows streamed whole against QT queries in LDS (lds_q[q * nvec + v]), software-pipelined: the loads of slice c + 1 are in
// flight while slice c is scored.  Whole slices run without any masking; only a ragged last slice (the row is not a
// multiple of the lane group) clamps its address and zeroes the operands of the lanes past the end
template <typename T, int METRIC, int QT, int R>
__device__ __forceinline__ void stream_rows(PairAcc<T, METRIC> (&acc)[R][QT], const char *const (&rp)[R], const Raw16 *lds_q,
                                            const LaneSplit &ls, int nvec, int lpr_log2, int nchunks) {
    const int nfull = nvec >> lpr_log2;
    auto score = [&](const Raw16(&rowv)[R], int vq, bool ok, auto masked) {
#pragma unroll
        for (int q = 0; q < QT; q++) {
            const Raw16 qv = lds_q[q * nvec + vq];
#pragma unroll
            for (int r = 0; r < R; r++) acc[r][q].template add<decltype(masked)::value>(rowv[r], qv, ok);
        }
    };
    Raw16 cur[R], nxt[R];
    {
        const int vi = ls.sub < nvec ? ls.sub : nvec - 1;
#pragma unroll
        for (int r = 0; r < R; r++) cur[r] = load16(rp[r] + (size_t)vi * sizeof(Raw16));
    }
    for (int c = 0; c < nfull; c++) {
        const int vi = c * ls.lpr + ls.sub;
        int vn = vi + ls.lpr;
        vn = vn < nvec ? vn : nvec - 1;
#pragma unroll
        for (int r = 0; r < R; r++) nxt[r] = load16(rp[r] + (size_t)vn * sizeof(Raw16));
        score(cur, vi, true, std::false_type{});
#pragma unroll
        for (int r = 0; r < R; r++) cur[r] = nxt[r];
    }
    if (nfull < nchunks) {
        const int vi = nfull * ls.lpr + ls.sub;
        const bool ok = vi < nvec;
        score(cur, ok ? vi : nvec - 1, ok, std::true_type{});
    }
}

// A persistent workgroup's next task from the device counter, through *lds_task: counter[0] counts claimed tasks,
// counter[1] the workgroups that found none left.  Every workgroup ends there exactly once, and the last one leaves both
// words zero for the next launch (no memset launch per scan: k-means++ issues one scan per center).  false: return
__device__ __forceinline__ bool pull_task(int *task_counter, int ntasks, int *lds_task, int *task) {
    if (threadIdx.x == 0) *lds_task = atomicAdd(task_counter, 1);
    __syncthreads();
    *task = *lds_task;
    if (*task < ntasks) return true;
    if (threadIdx.x == 0 && atomicAdd(task_counter + 1, 1) == (int)gridDim.x - 1) {
        atomicExch(task_counter + 1, 0);
        atomicExch(task_counter, 0);
    }
    return false;
}

}  // namespace pgv
