// kernels_bit.hip -- binary quantization on the device: the two-stage query of the reference's README,
//     SELECT * FROM (SELECT * FROM items ORDER BY binary_quantize(embedding)::bit(d) <~> binary_quantize($1) LIMIT k')
//     ORDER BY embedding <=> $1 LIMIT k
// for a batch of queries.
//   hamming_tile_kernel      hamming_distance (src/bitvec.c:45-56 over BitHammingDistanceDefault, src/bitutils.c:49-73)
//                            of a tile of rows against a tile of queries, into pgv_bit_topk's distance matrix
//   binary_quantize_kernel   binary_quantize (src/vector.c:952-979, halfvec_binary_quantize in src/halfvec.c)
//   rerank_*_kernel          what pgv_rerank needs around score_gather_kernel and topk_kernel
// bit_kernel (kernels_misc.hip) stays the operator path: one query, float8 out, both bit metrics.
//
// hamming_tile_kernel: 256 rows x 32 queries per workgroup, one lane per row.
//   * the rows leave HBM once per 32 queries: 8 adjacent lanes fetch 128 contiguous bytes of one row with 16-byte loads,
//     the slice goes through LDS (row stride 9 vectors: lane i's ds_read_b128 at 36 i words hits 16 distinct 4-bank
//     slots in each of the instruction's 16-lane groups) and comes back as 32 words of the lane's own row in registers
//   * the query words are the same for every lane: they are read through the scalar cache into SGPRs, so the inner
//     step per word is v_xor_b32 with a scalar operand and v_bcnt_u32_b32 accumulating into an integer register
//   * rows longer than the register slice (kBitSliceBits) are walked slice by slice, the next slice's global loads in
//     flight while the current one is counted; the 32 counts per lane are converted to float once, at the store
//   * stores are coalesced along `row`: lane i writes out[q * n + row0 + i]
// Rows are padded with zero bytes to whole 16-byte vectors and queries to whole slices (pgv_bit_topk stages them):
// padding adds nothing to a count.  Tail rows and tail queries clamp their address and are computed, not stored.
#include "pgv_device.h"

namespace pgv {

namespace {

constexpr int kBitThreads = 256;                            // rows per tile
constexpr int kBitQueries = 32;                             // queries per tile
constexpr int kBitSliceVecs = 8;                            // 16-byte vectors of a row in registers at a time
constexpr int kBitSliceWords = kBitSliceVecs * 4;           // 32
constexpr int kBitSliceBits = kBitSliceWords * 32;          // 1024: the register slice
constexpr int kBitLdsStride = kBitSliceVecs + 1;            // vectors; the pad keeps the transposed read conflict-free
constexpr int kBitRowsPerTrip = kBitThreads / kBitSliceVecs;  // 32 rows per cooperative load instruction
static_assert(kBitSliceBits == 1024, "tests/test_gpu_bit_topk.py sweeps nbits around the register slice");

__global__ __launch_bounds__(kBitThreads) void hamming_tile_kernel(const char *__restrict__ rows,
                                                                   const uint32_t *__restrict__ queries, int64_t n, int nq,
                                                                   int nvec, int qwords, int nqt, float *__restrict__ out) {
    __shared__ Raw16 tile[kBitThreads * kBitLdsStride];
    const int tid = threadIdx.x;
    // consecutive workgroups share a row tile: its query tiles run side by side and find the rows in the caches
    const int qt = (int)(blockIdx.x % (unsigned)nqt);
    const int64_t row0 = (int64_t)(blockIdx.x / (unsigned)nqt) * kBitThreads;
    const int q0 = qt * kBitQueries;
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
            int64_t r = row0 + lr + i * kBitRowsPerTrip;
            r = r < n ? r : n - 1;  // tail rows are computed, not stored
            const Raw16 v = load16(rows + (size_t)r * row_bytes + (size_t)vc * sizeof(Raw16));
            nxt[i] = ok ? v : raw16_zero();
        }
    };

    int acc[kBitQueries];
#pragma unroll
    for (int q = 0; q < kBitQueries; q++) acc[q] = 0;

    fetch(0);
    for (int s = 0; s < nslices; s++) {
        __syncthreads();  // every lane has its words of the slice before
#pragma unroll
        for (int i = 0; i < kBitSliceVecs; i++) tile[(lr + i * kBitRowsPerTrip) * kBitLdsStride + lv] = nxt[i];
        __syncthreads();
        Raw16 rv[kBitSliceVecs];
#pragma unroll
        for (int v = 0; v < kBitSliceVecs; v++) rv[v] = tile[tid * kBitLdsStride + v];
        if (s + 1 < nslices) fetch(s + 1);

        const uint32_t *qs = queries + (size_t)s * kBitSliceWords;
#pragma unroll
        for (int q = 0; q < kBitQueries; q++) {
            const int qi = q0 + q < nq ? q0 + q : nq - 1;  // tail queries are computed, not stored
            const uint32_t *qp = qs + (size_t)qi * qwords;  // wave-uniform: scalar loads
#pragma unroll
            for (int v = 0; v < kBitSliceVecs; v++)
#pragma unroll
                for (int w = 0; w < 4; w++) acc[q] = __popc(rv[v].w[w] ^ qp[v * 4 + w]) + acc[q];
        }
    }

    const int64_t row = row0 + tid;
    if (row < n) {
#pragma unroll
        for (int q = 0; q < kBitQueries; q++)
            if (q0 + q < nq) out[(size_t)(q0 + q) * (size_t)n + (size_t)row] = (float)acc[q];
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

// pgv_rerank: candidate lists [nq x kc] -> the pairs score_gather_kernel reads.  "none" (-1) scores row 0 of the pair's
// query; rerank_mask_kernel overwrites the value
__global__ void rerank_pairs_kernel(const int64_t *__restrict__ cand, int64_t total, int kc, int32_t *__restrict__ slot,
                                    int32_t *__restrict__ query_of) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t c = cand[i];
    slot[i] = c < 0 ? 0 : (int32_t)c;
    query_of[i] = (int32_t)(i / kc);
}

__global__ void rerank_mask_kernel(const int64_t *__restrict__ cand, int64_t total, float *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total && cand[i] < 0) vals[i] = INFINITY;
}

// position inside a query's candidate list -> the row index the list holds there
__global__ void rerank_map_kernel(const int64_t *__restrict__ cand, int nq, int kc, int k, const int64_t *__restrict__ pos,
                                  int64_t *__restrict__ out_idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)nq * k) return;
    const int64_t p = pos[i];
    int64_t c = p < 0 ? -1 : cand[(i / k) * kc + p];
    out_idx[i] = c < 0 ? -1 : c;
}

}  // namespace

int bit_topk_slice_bytes() { return kBitSliceVecs * (int)sizeof(Raw16); }

int launch_hamming_tiles(pgv_ctx *ctx, const void *rows, int nvec, int64_t n, const void *queries, int qbytes, int nq,
                         float *out) {
    if (n <= 0 || nq <= 0) return PGV_OK;
    const int nqt = (nq + kBitQueries - 1) / kBitQueries;
    const int64_t grid = (n + kBitThreads - 1) / kBitThreads * nqt;
    if (grid > 0x7fffffff) PGV_FAIL(PGV_ERR_ARG, "bit scan: too many tiles");
    hipLaunchKernelGGL(hamming_tile_kernel, dim3((unsigned)grid), dim3(kBitThreads), 0, ctx->stream,
                       static_cast<const char *>(rows), static_cast<const uint32_t *>(queries), n, nq, nvec, qbytes / 4, nqt,
                       out);
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

int launch_rerank_pairs(pgv_ctx *ctx, const int64_t *cand, int64_t total, int kc, int32_t *slot, int32_t *query_of) {
    if (total <= 0) return PGV_OK;
    hipLaunchKernelGGL(rerank_pairs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, cand, total, kc,
                       slot, query_of);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_rerank_mask(pgv_ctx *ctx, const int64_t *cand, int64_t total, float *vals) {
    if (total <= 0) return PGV_OK;
    hipLaunchKernelGGL(rerank_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, cand, total,
                       vals);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_rerank_map(pgv_ctx *ctx, const int64_t *cand, int nq, int kc, int k, const int64_t *pos, int64_t *out_idx) {
    const int64_t total = (int64_t)nq * k;
    if (total <= 0) return PGV_OK;
    hipLaunchKernelGGL(rerank_map_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, cand, nq, kc, k,
                       pos, out_idx);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

}  // namespace pgv
