// kernels_cosine.hip -- pgv_cosine_topk: every query x every row under cosine_distance as the operator computes it
// (src/vector.c:649-697, src/halfvec.c:652-700), rows as the table stores them, and a top-k that is exact in the float8.
//
//   cosine_tile_kernel<T>   128 queries x 128 rows per workgroup on the matrix cores (mfma_dense_kernel's geometry,
//                           staging and swizzle, kernels_dense.hip).  The reference's loop has three accumulators:
//                           similarity, norma, normb.  The first is the MFMA accumulator; the other two are summed from
//                           the SAME operand registers the lane has just read for the MFMAs, so the rows are read from
//                           HBM once and no norms pass runs in front.  Per pair the epilogue evaluates
//                             d = 1 - clamp((double) ip / sqrt((double) na * (double) nb), -1, 1)        (cosine_value)
//                           and stores two floats: IP (the inner product, what d is recomputed from later) and KEY, d
//                           truncated to float precision (cosine_key): monotone in d, so the float selection kernels
//                           order it correctly but coarsely.
//   cosine_settle_kernel    after launch_topk_segments(KEY, k + 1): is the boundary's key class inside the selection?
//   cosine_refine_kernel    for the queries where it is not: the row of KEY is rewritten so that a second float
//                           selection separates the boundary class by the low 29 mantissa bits of d
//   cosine_finish_kernel    d of the selected pairs again (the same function: the same bits), sorted by (d, index)
//
// A value depends on the pair and dim only: one kernel serves every nq and n (a short tile is padded by repeating its
// last row), a lane's partial norm runs over the slices in order, the two half-waves' partials are added once at the
// end, and the inner product is one accumulator chain in the matrix pipeline.  Nothing depends on the tile a row or a
// query falls into.
#include "pgv_device.h"
#include "pgv_internal.h"

namespace pgv {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kCosSlice = 128;                        // bytes of a row per stage
constexpr int kCosTile = 128;                         // queries and rows per workgroup
constexpr int kCosStage = 2 * kCosTile * kCosSlice;   // 32 KB: [128 query rows | 128 data rows] x 128 B
constexpr int kCosThreads = 256;

// cosine_distance of one pair from the three fp32 sums: `Use sqrt(a * b) over sqrt(a) * sqrt(b)` (vector.c:664-665), the
// clamp of :688-694.  NaN (a zero vector: 0 / 0; an overflowed product: inf / inf) passes through both comparisons.
// The result is +0, a double in [2^-53, 2], or NaN
__device__ __forceinline__ double cosine_value(float ip, float na, float nb) {
    double s = (double)ip / sqrt((double)na * (double)nb);
    if (s > 1.0)
        s = 1.0;
    else if (s < -1.0)
        s = -1.0;
    return 1.0 - s;
}

// The order image of d for the float selection: d truncated (not rounded) to a float -- the double's exponent rebased,
// its top 23 mantissa bits kept.  2^-53 <= d <= 2 lands in the normal floats, 0 stays 0, NaN stays NaN; the image is
// monotone non-decreasing in d, and two values with one image differ in the low 29 mantissa bits only (cosine_low)
constexpr unsigned long long kCosRebase = (unsigned long long)(1023 - 127) << 23;
constexpr unsigned kCosLowMask = (1u << 29) - 1;
__device__ __forceinline__ float cosine_key(double d) {
    if (d != d) return __uint_as_float(0x7fc00000u);
    if (d == 0.0) return 0.f;
    return __uint_as_float((unsigned)(((unsigned long long)__double_as_longlong(d) >> 29) - kCosRebase));
}
__device__ __forceinline__ unsigned cosine_low(double d) { return (unsigned)__double_as_longlong(d) & kCosLowMask; }

// positive finite floats order as their patterns (jaccard_image's device, pgv_device.h): the refined images
constexpr unsigned kCosImageBelow = 0x00800000u;  // every row under the boundary class: the smallest normal float
constexpr unsigned kCosImageClass = 0x00800001u;  // + cosine_low(d): at most 0x20800000, finite

template <typename T> struct CosMma;
template <> struct CosMma<float> {
    static __device__ __forceinline__ void run(f32x16 &acc, const u32x4 &a, const u32x4 &b) {
#pragma unroll
        for (int e = 0; e < 4; e++)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[e]), __uint_as_float(b[e]), acc, 0, 0, 0);
    }
    // norma += ax[i] * ax[i] over the 4 elements of one operand
    static __device__ __forceinline__ void square(float &s, const u32x4 &v) {
#pragma unroll
        for (int e = 0; e < 4; e++) s = __builtin_fmaf(__uint_as_float(v[e]), __uint_as_float(v[e]), s);
    }
};
template <> struct CosMma<__half> {
    static __device__ __forceinline__ void run(f32x16 &acc, const u32x4 &a, const u32x4 &b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0,
                                                     0, 0);
    }
    // ... over the 8: the products of two halves are exact in fp32, a packed dot adds two of them to the sum
    static __device__ __forceinline__ void square(float &s, const u32x4 &v) {
        const f16x8 h = __builtin_bit_cast(f16x8, v);
        const f16x2 h0 = __builtin_shufflevector(h, h, 0, 1), h1 = __builtin_shufflevector(h, h, 2, 3);
        const f16x2 h2 = __builtin_shufflevector(h, h, 4, 5), h3 = __builtin_shufflevector(h, h, 6, 7);
        s = __builtin_amdgcn_fdot2(h0, h0, s, false);
        s = __builtin_amdgcn_fdot2(h1, h1, s, false);
        s = __builtin_amdgcn_fdot2(h2, h2, s, false);
        s = __builtin_amdgcn_fdot2(h3, h3, s, false);
    }
};

// ip_out / key_out[q * n + r] for q in [0, nq), r in [0, n); na_out[q], nb_out[r]: the squared norms, written by the
// workgroups of row tile 0 / query tile 0 (every workgroup that holds one computes the same bits).  Grid and the walk
// over the XCDs are mfma_dense_kernel's: 8 * ceil(row_tiles / 8) * qtiles workgroups, the qtiles workgroups of one row
// tile consecutive on one XCD.
template <typename T>
__global__ __launch_bounds__(kCosThreads, 2) void cosine_tile_kernel(const char *__restrict__ rows, int64_t n,
                                                                      const char *__restrict__ queries, int nq, int nvec,
                                                                      const char *__restrict__ zeros16,
                                                                      float *__restrict__ ip_out,
                                                                      float *__restrict__ key_out,
                                                                      float *__restrict__ na_out,
                                                                      float *__restrict__ nb_out, int qtiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;  // 2 x 2 wavefronts, 64 queries x 64 rows each
    const int l31 = lane & 31, half = lane >> 5;
    const unsigned sw = (unsigned)(l31 >> 1) & 7u;

    const int64_t w = blockIdx.x, x = w & 7, sq = w >> 3;
    const int qt = (int)(sq % qtiles);
    const int64_t row_tile = x + 8 * (sq / qtiles);
    const int64_t row_base = row_tile * kCosTile;
    if (row_base >= n) return;  // the padded tail of the XCD round-robin
    const int q_base = qt * kCosTile;
    const size_t row_bytes = (size_t)nvec * sizeof(Raw16);
    const int nslices = (nvec + 7) / 8;

    // DMA role: this wavefront fills 64 consecutive rows of the concatenation [128 query rows | 128 data rows], 8 per
    // instruction; a lane brings slot (lane & 7) of row (lane >> 3) of its group.  Rows past the end repeat the last one:
    // that is the padding of a short tile, whose values are never stored.
    const int crow0 = wave * 64;
    const bool fills_q = crow0 < kCosTile;
    const int drow = lane >> 3, dpos = lane & 7;
    const char *src_base = fills_q ? queries + (size_t)q_base * row_bytes : rows + (size_t)row_base * row_bytes;
    const int64_t src_limit = fills_q ? (int64_t)(nq - q_base < kCosTile ? nq - q_base : kCosTile)
                                      : (n - row_base < kCosTile ? n - row_base : kCosTile);
    const char *src[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int64_t i = (fills_q ? crow0 : crow0 - kCosTile) + 8 * j + drow;
        src[j] = src_base + (size_t)(i < src_limit ? i : src_limit - 1) * row_bytes;
    }
    auto issue_stage = [&](int sl, int buf) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int v = dpos ^ ((4 * j + (drow >> 1)) & 7);  // slot p of row i holds vector p ^ ((i >> 1) & 7)
            const int vi = sl * 8 + v;
            const char *p = vi < nvec ? src[j] + (size_t)vi * sizeof(Raw16) : zeros16;
            char *dst = smem + (size_t)buf * kCosStage + (size_t)(crow0 + 8 * j) * kCosSlice;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)p,
                                             (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;
    // this lane's share of |query|^2 (query wm * 64 + tm * 32 + l31) and |row|^2 (row wn * 64 + tn * 32 + l31): the
    // vectors 2 c + half of every slice, in order; the other half-wave holds the rest of the same rows
    float pa[2] = {0.f, 0.f}, pb[2] = {0.f, 0.f};

    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
    const unsigned a_lane = (unsigned)(wm * 64 + l31) * kCosSlice;
    const unsigned b_lane = (unsigned)(kCosTile + wn * 64 + l31) * kCosSlice;

    issue_stage(0, 0);
    for (int sl = 0; sl < nslices; sl++) {
        // the slice has landed for every wavefront and nobody still reads the other buffer (the wait is spelled out:
        // __syncthreads() alone does not drain an LDS-DMA)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (sl + 1 < nslices) issue_stage(sl + 1, (sl + 1) & 1);
        const unsigned sbase = lds0 + (unsigned)(sl & 1) * kCosStage;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const unsigned xo = (((unsigned)(2 * c + half)) ^ sw) << 4;
            u32x4 a[2], b[2];
            asm volatile(
                "ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:4096\n\t"
                "ds_read_b128 %2, %5\n\tds_read_b128 %3, %5 offset:4096\n\t"
                "s_waitcnt lgkmcnt(0)"
                : "=&v"(a[0]), "=&v"(a[1]), "=&v"(b[0]), "=&v"(b[1])
                : "v"(sbase + a_lane + xo), "v"(sbase + b_lane + xo)
                : "memory");
#pragma unroll
            for (int tm = 0; tm < 2; tm++)
#pragma unroll
                for (int tn = 0; tn < 2; tn++) CosMma<T>::run(acc[tm][tn], a[tm], b[tn]);
#pragma unroll
            for (int t = 0; t < 2; t++) {
                CosMma<T>::square(pa[t], a[t]);
                CosMma<T>::square(pb[t], b[t]);
            }
        }
    }
    // the two half-waves' partials, added once: p + p' in one half and p' + p in the other are the same bits
    float na[2], nb[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        na[t] = pa[t] + __shfl_xor(pa[t], 32);
        nb[t] = pb[t] + __shfl_xor(pb[t], 32);
    }
    // nb sits in the lane that owns the row below; the 128 na go through LDS once (the stage buffers are free when
    // every wavefront has left the loop)
    float *na_s = reinterpret_cast<float *>(smem);
    __syncthreads();
    if (wn == 0 && half == 0) {
#pragma unroll
        for (int tm = 0; tm < 2; tm++) {
            const int ql = wm * 64 + tm * 32 + l31;
            na_s[ql] = na[tm];
            if (row_tile == 0 && q_base + ql < nq) na_out[q_base + ql] = na[tm];
        }
    }
    __syncthreads();

    // a lane holds, per tile, 16 queries' values for ONE row: register e is query (e & 3) + 8 (e >> 2) + 4 half; the 32
    // lanes of a half-wave write 32 consecutive rows of one query: 128-byte stores, twice
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        const int64_t r = row_base + wn * 64 + tn * 32 + l31;
        if (r >= n) continue;
        if (qt == 0 && wm == 0 && half == 0) nb_out[r] = nb[tn];
#pragma unroll
        for (int tm = 0; tm < 2; tm++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int ql = wm * 64 + tm * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
                const int q = q_base + ql;
                if (q >= nq) continue;
                const float ip = acc[tm][tn][e];
                const size_t at = (size_t)q * (size_t)n + (size_t)r;
                ip_out[at] = ip;
                key_out[at] = cosine_key(cosine_value(ip, na_s[ql], nb[tn]));
            }
    }
}

// sel_val [nq x kk]: the kk smallest keys of every query, ascending (launch_topk_segments).  A query is settled when the
// selection holds every row (kk == n), or when entry k exists and its key is strictly above entry k - 1's: the key class
// of the boundary then ends inside the first k entries, which are the exact set.  Otherwise kb = the boundary's key and
// *count goes up (zero before the launch)
__global__ void cosine_settle_kernel(const float *__restrict__ sel_val, int nq, int kk, int k, int64_t n,
                                     float *__restrict__ kb, int *__restrict__ unsettled, int *__restrict__ count) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const float *v = sel_val + (size_t)q * kk;
    const bool settled = kk == n || (kk == k + 1 && float_to_key(v[k]) > float_to_key(v[k - 1]));
    unsettled[q] = settled ? 0 : 1;
    kb[q] = settled ? 0.f : v[k - 1];
    if (!settled) atomicAdd(count, 1);
}

// An unsettled query's row of KEY, in place, per_query workgroups a query: under the class -> the smallest image, above
// it (NaN included) -> +inf, inside it -> kCosImageClass + the low 29 mantissa bits of d, recomputed from IP and the
// norms (the rows of a class share every higher bit of d, so these order as d does).  A NaN class has no d to order:
// one common image, the ties go by index.  The k smallest of the rewritten row are the exact set
__global__ __launch_bounds__(kCosThreads) void cosine_refine_kernel(float *__restrict__ key, const float *__restrict__ ip,
                                                                    const float *__restrict__ na,
                                                                    const float *__restrict__ nb,
                                                                    const float *__restrict__ kb,
                                                                    const int *__restrict__ unsettled, int64_t n,
                                                                    int per_query) {
    const int q = blockIdx.x / per_query, part = blockIdx.x % per_query;
    if (!unsettled[q]) return;
    const unsigned kbk = float_to_key(kb[q]);
    const bool nan_class = kbk == 0xffffffffu;
    const float naq = na[q];
    float *krow = key + (size_t)q * (size_t)n;
    const float *iprow = ip + (size_t)q * (size_t)n;
    for (int64_t r = (int64_t)part * kCosThreads + threadIdx.x; r < n; r += (int64_t)per_query * kCosThreads) {
        const unsigned kr = float_to_key(krow[r]);
        unsigned image;
        if (kr < kbk)
            image = kCosImageBelow;
        else if (kr > kbk)
            image = 0x7f800000u;
        else
            image = nan_class ? kCosImageClass : kCosImageClass + cosine_low(cosine_value(iprow[r], naq, nb[r]));
        krow[r] = __uint_as_float(image);
    }
}

// One workgroup a query: d of the selected rows (pos [nq x pos_stride], the first `take` of a row: the exact set, or
// every row when the selection holds them all -- then the float8 order decides which k leave), sorted by (d, index) in
// LDS -- positive doubles order as their patterns, every NaN becomes one pattern above them, the padding sits above
// that -- then the first k go to out_dist / out_idx [nq x k], +inf / -1 behind.  kp: a power of two >= max(k, take, 2)
__global__ __launch_bounds__(kCosThreads) void cosine_finish_kernel(const float *__restrict__ ip,
                                                                    const float *__restrict__ na,
                                                                    const float *__restrict__ nb,
                                                                    const int64_t *__restrict__ pos, int pos_stride,
                                                                    int take, int64_t n, int k, int kp,
                                                                    double *__restrict__ out_dist,
                                                                    int64_t *__restrict__ out_idx) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long *img = reinterpret_cast<unsigned long long *>(smem);  // [kp]
    unsigned *idx = reinterpret_cast<unsigned *>(img + kp);                  // [kp]
    constexpr unsigned long long kNan = 0x7ff8000000000000ull, kPad = ~0ull;
    const int q = blockIdx.x;
    for (int i = threadIdx.x; i < kp; i += kCosThreads) {
        unsigned long long im = kPad;
        unsigned ix = 0xffffffffu;
        const int64_t p = i < take ? pos[(size_t)q * pos_stride + i] : -1;
        if (p >= 0 && p < n) {
            const double d = cosine_value(ip[(size_t)q * (size_t)n + (size_t)p], na[q], nb[p]);
            im = d != d ? kNan : (unsigned long long)__double_as_longlong(d);
            ix = (unsigned)p;
        }
        img[i] = im;
        idx[i] = ix;
    }
    // bitonic network over (img, idx), ascending
    for (int size = 2; size <= kp; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < kp / 2; t += kCosThreads) {
                const int lo = t & (stride - 1);
                const int i = ((t - lo) << 1) + lo, j = i + stride;
                const unsigned long long a = img[i], b = img[j];
                const unsigned ai = idx[i], bi = idx[j];
                const bool after = a > b || (a == b && ai > bi);  // i's entry belongs behind j's
                if (after == ((i & size) == 0)) {
                    img[i] = b;
                    img[j] = a;
                    idx[i] = bi;
                    idx[j] = ai;
                }
            }
        }
    __syncthreads();
    for (int i = threadIdx.x; i < k; i += kCosThreads) {
        const unsigned long long im = img[i];
        out_dist[(size_t)q * k + i] = im == kPad ? (double)INFINITY : __longlong_as_double((long long)im);
        out_idx[(size_t)q * k + i] = im == kPad ? -1 : (int64_t)idx[i];
    }
}

}  // namespace

int launch_cosine_tiles(pgv_ctx *ctx, pgv_dtype dtype, const RowGeom &g, const void *rows, int64_t n, const void *queries,
                        int nq, float *ip, float *key, float *na, float *nb) {
    if (n <= 0 || nq <= 0) return PGV_OK;
    if (!ctx->zeros.p) {
        PGV_TRY(ctx->zeros.ensure(256));
        PGV_HIP(hipMemsetAsync(ctx->zeros.p, 0, 256, ctx->stream));
    }
    const int qtiles = (nq + kCosTile - 1) / kCosTile;
    const int64_t row_tiles = (n + kCosTile - 1) / kCosTile;
    const int64_t grid = 8 * ((row_tiles + 7) / 8) * qtiles;
    if (grid > 0x7fffffff) PGV_FAIL(PGV_ERR_ARG, "cosine scan: too many workgroups");
    const size_t lds = 2 * (size_t)kCosStage;
#define PGV_COSINE(T)                                                                                                     \
    {                                                                                                                     \
        auto kern = cosine_tile_kernel<T>;                                                                                \
        PGV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,     \
                                    (int)lds));                                                                           \
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kCosThreads), lds, ctx->stream,                               \
                           static_cast<const char *>(rows), n, static_cast<const char *>(queries), nq, g.nvec,            \
                           static_cast<const char *>(ctx->zeros.p), ip, key, na, nb, qtiles);                             \
    }
    if (dtype == PGV_F32) PGV_COSINE(float) else PGV_COSINE(__half)
#undef PGV_COSINE
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_cosine_settle(pgv_ctx *ctx, const float *sel_val, int nq, int kk, int k, int64_t n, float *kb, int *unsettled,
                         int *count) {
    if (nq <= 0) return PGV_OK;
    PGV_HIP(hipMemsetAsync(count, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(cosine_settle_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, sel_val, nq, kk,
                       k, n, kb, unsettled, count);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_cosine_refine(pgv_ctx *ctx, float *key, const float *ip, const float *na, const float *nb, const float *kb,
                         const int *unsettled, int nq, int64_t n) {
    if (nq <= 0 || n <= 0) return PGV_OK;
    // nq * n stays within the chunk's matrix, so nq * per_query does within a grid
    const int per_query = (int)std::min<int64_t>((n + 4 * kCosThreads - 1) / (4 * kCosThreads), 64);
    hipLaunchKernelGGL(cosine_refine_kernel, dim3((unsigned)((int64_t)nq * per_query)), dim3(kCosThreads), 0, ctx->stream,
                       key, ip, na, nb, kb, unsettled, n, per_query);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_cosine_finish(pgv_ctx *ctx, const float *ip, const float *na, const float *nb, const int64_t *pos,
                         int pos_stride, int take, int nq, int64_t n, int k, double *out_dist, int64_t *out_idx) {
    if (nq <= 0) return PGV_OK;
    if (take < 0 || take > 4096 || take > pos_stride) PGV_FAIL(PGV_ERR_ARG, "cosine finish: %d positions a query", take);
    int kp = 2;
    while (kp < k || kp < take) kp <<= 1;
    const size_t lds = (size_t)kp * (sizeof(unsigned long long) + sizeof(unsigned));
    hipLaunchKernelGGL(cosine_finish_kernel, dim3((unsigned)nq), dim3(kCosThreads), lds, ctx->stream, ip, na, nb, pos,
                       pos_stride, take, n, k, kp, out_dist, out_idx);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

}  // namespace pgv
