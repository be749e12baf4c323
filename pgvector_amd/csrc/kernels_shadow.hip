// kernels_shadow.hip -- the fp16 residual shadow of an fp32 L2 index and the per-batch terms of its list scan.
//
// The batched MFMA list scan of an L2 index only PRE-FILTERS: batch_recheck_kernel recomputes the reference's exact
// sum((q - x)^2) over the fp32 rows for the candidates inside a proven rounding band.  The pre-filter
// therefore need not read the fp32 rows.  It reads a shadow of half the bytes instead:
//
//   x = c_l + rho            (c_l: the center of the row's list)
//   shadow row  = fp16(rho * 2^-s)          one power-of-two scale s per index: the largest |rho_i| lands near 2^14
//   query row   = fp16(q * 2^-s_q)          one power-of-two scale s_q per query, cast once per batch
//   pair term t = -2 q.c_l                  fp32, once per probed (query, list) pair
//   value       = |x|^2 + t - 2^(1 + s + s_q) (shadow_q . shadow_x)
//
// which is the same quantity |x|^2 - 2 q.x the fp32 scan computes, up to an error that the query-cast kernel bounds
// per query (shadow_query_kernel; the derivation is next to ScanBound in pgv_internal.h).  E and P of the index
// (largest |rho - 2^s shadow| and largest |2^s shadow| over its rows) are measured here when the shadow is written,
// so the bound holds whatever the data: subnormals, huge values and uneven lists only widen the band.
#include "pgv_device.h"

#include <cfloat>

namespace pgv {

namespace {

// the list of row r: last l with list_off[l] <= r (empty lists share an offset with the next one)
__device__ __forceinline__ int list_of_row(const int64_t *__restrict__ list_off, int nlists, int64_t r) {
    int lo = 0, hi = nlists - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (list_off[mid] <= r)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// 2^e - 14 scale of a largest magnitude m: m * 2^-s lies in (2^13, 2^14] (0 / non-finite: s = 0)
__device__ __forceinline__ int scale_for(float m) {
    if (!(m > 0.f) || !isfinite(m)) return 0;
    int e;
    (void)frexpf(m, &e);  // m = f 2^e, f in [0.5, 1)
    return e - 14;
}

// pass 1: the largest |x_i - c_i| over the index (bits of a non-negative float: integer order is float order).
// centers == null: the rows are cast as they are (c = 0; the shadow of the centers themselves, launch_shadow_build)
__global__ __launch_bounds__(256) void shadow_absmax_kernel(const float *__restrict__ rows, const float *__restrict__ centers,
                                                            const int64_t *__restrict__ list_off, int nlists, int64_t n,
                                                            int ld, unsigned *__restrict__ max_bits) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int lane = threadIdx.x & (kWave - 1);
    const float *x = rows + (size_t)r * ld;
    const float *c = centers ? centers + (size_t)list_of_row(list_off, nlists, r) * ld : nullptr;
    float m = 0.f;
    for (int i = lane; i < ld; i += kWave) {
        const float d = fabsf(c ? x[i] - c[i] : x[i]);
        m = (d > m || d != d) ? d : m;  // (NaN is kept: its bits compare above every number)
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float v = __shfl_xor(m, o);
        m = (v > m || v != v) ? v : m;
    }
    if (lane == 0 && __float_as_uint(m) > __hip_atomic_load(max_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(max_bits, __float_as_uint(m));
}

// pass 2: the shadow rows, and per row |rho - 2^s shadow|^2 and |2^s shadow|^2 in fp64 (maxima as bits of
// non-negative doubles).  rho is formed in fp64 too: the difference of two floats is exact there unless their
// exponents lie ~30 apart (the host adds 2^-40 P for that)
__global__ __launch_bounds__(256) void shadow_build_kernel(const float *__restrict__ rows, const float *__restrict__ centers,
                                                           const int64_t *__restrict__ list_off, int nlists, int64_t n,
                                                           int ld, int ld16, const unsigned *__restrict__ max_bits,
                                                           __half *__restrict__ shadow,
                                                           unsigned long long *__restrict__ ep_bits,
                                                           unsigned long long *__restrict__ radius_bits) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int s = scale_for(__uint_as_float(*max_bits));
    const float *x = rows + (size_t)r * ld;
    const int list = centers ? list_of_row(list_off, nlists, r) : 0;
    const float *c = centers ? centers + (size_t)list * ld : nullptr;
    __half *h = shadow + (size_t)r * ld16;
    const double up = ldexp(1.0, s);  // (exact: |s| stays far inside fp64's exponent range)
    double e2 = 0.0, p2 = 0.0, r2 = 0.0;  // r2 = |x - c_l|^2: the list's radius (probe pruning, pgv_internal.h)
    for (int i = lane; i < ld16; i += kWave) {
        __half v = __float2half(0.f);
        if (i < ld) {
            const float ci = c ? c[i] : 0.f;
            v = __float2half(ldexpf(x[i] - ci, -s));
            const double back = (double)__half2float(v) * up;
            const double rho = (double)x[i] - (double)ci;
            const double d = rho - back;
            r2 = fma(rho, rho, r2);
            e2 = fma(d, d, e2);
            p2 = fma(back, back, p2);
        }
        h[i] = v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        e2 += __shfl_xor(e2, o);
        p2 += __shfl_xor(p2, o);
        r2 += __shfl_xor(r2, o);
    }
    if (lane == 0) {
        // (NaN / inf rows: the host finds a non-finite E or P and drops the shadow).  A million atomics on one word take
        // ~11 ms: nearly every row is below the maximum seen so far and only looks
        const unsigned long long eb = (unsigned long long)__double_as_longlong(e2 != e2 ? INFINITY : e2),
                                 pb = (unsigned long long)__double_as_longlong(p2 != p2 ? INFINITY : p2);
        if (eb > __hip_atomic_load(&ep_bits[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&ep_bits[0], eb);
        if (pb > __hip_atomic_load(&ep_bits[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&ep_bits[1], pb);
        if (radius_bits) {  // one word per list, the same way
            const unsigned long long rb = (unsigned long long)__double_as_longlong(r2 != r2 ? INFINITY : r2);
            if (rb > __hip_atomic_load(&radius_bits[list], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(&radius_bits[list], rb);
        }
    }
}

// One wavefront per query: the fp16 query row 2^-s_q q (scale per query), the epilogue's factor 2^(1 + s + s_q), and
// the additive term of the rounding band that the shadow adds (pgv_internal.h, ScanBound).  The terms are formed in
// fp64 and rounded up into fp32.  One cast serves both consumers of a batch: cscale / ceps (null: not wanted) are the
// factor 2^(1 + s_c + s_q) and the band term of the center ranking over the centers' shadow (RankShadowTerms), qscale /
// qeps (null: not wanted) those of the list scan.
//
// The row is read ONCE, with 16-byte loads, into registers: a lane owns chunks of 8 consecutive elements (two loads, one
// 16-byte store of fp16), kCastChunks of them cover rows up to 64 * 8 * kCastChunks = 2048 elements; a longer row is
// read twice, chunk by chunk (once for the maximum, once for the cast).  The maximum and the cast are per element, so
// the fp16 row and the power-of-two scales do not depend on which lane holds what.  The three fp64 sums run as four
// independent chains per lane (element e of a chunk feeds chain e & 3) in place of one chain of ld / 64 dependent
// FMAs; the order of summation differs from a single chain's, which the band terms allow: they are upper bounds formed
// in fp64 (relative error of any order of n additions <= n 2^-53) and inflated by 2^-20 before they are rounded up.
constexpr int kCastChunks = 4;

struct CastChunk {
    float4 a, b;
};

__device__ __forceinline__ float absmax_keep_nan(float m, float v) {
    const float a = fabsf(v);
    return (a > m || a != a) ? a : m;  // (NaN is kept: it poisons the scale's input, the band becomes infinite)
}

__device__ __forceinline__ CastChunk cast_chunk_load(const float *__restrict__ x, int c, int ld) {
    CastChunk r;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    // (ld is a multiple of 4, ld16 of 8: the second half of the last chunk may lie past the fp32 row)
    r.a = 8 * c < ld ? *reinterpret_cast<const float4 *>(x + 8 * c) : zero;
    r.b = 8 * c + 4 < ld ? *reinterpret_cast<const float4 *>(x + 8 * c + 4) : zero;
    return r;
}

__device__ __forceinline__ float cast_chunk_max(const CastChunk &r, float m) {
    m = absmax_keep_nan(m, r.a.x);
    m = absmax_keep_nan(m, r.a.y);
    m = absmax_keep_nan(m, r.a.z);
    m = absmax_keep_nan(m, r.a.w);
    m = absmax_keep_nan(m, r.b.x);
    m = absmax_keep_nan(m, r.b.y);
    m = absmax_keep_nan(m, r.b.z);
    m = absmax_keep_nan(m, r.b.w);
    return m;
}

// the chunk's eight fp16 values as one 16-byte store; the elements below ld feed the sums (those past it are padding: 0)
__device__ __forceinline__ void cast_chunk_store(const CastChunk &r, int c, int ld, int sq, double up, __half *__restrict__ h,
                                                 double (&qq)[4], double (&dd)[4], double (&hh)[4]) {
    const float xs[8] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w};
    union {
        __half v[8];
        uint4 w;
    } out;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        __half v = __float2half(0.f);
        if (8 * c + e < ld) {
            v = __float2half(ldexpf(xs[e], -sq));
            const double back = (double)__half2float(v) * up, xi = (double)xs[e];
            qq[e & 3] = fma(xi, xi, qq[e & 3]);
            dd[e & 3] = fma(xi - back, xi - back, dd[e & 3]);  // (xi - back: exact in fp64)
            hh[e & 3] = fma(back, back, hh[e & 3]);
        }
        out.v[e] = v;
    }
    *reinterpret_cast<uint4 *>(h + 8 * c) = out.w;
}

__global__ __launch_bounds__(256) void shadow_query_kernel(const float *__restrict__ queries, int nq, int ld, int ld16,
                                                           ShadowTerms st, RankShadowTerms rt,
                                                           const float *__restrict__ center_norm_max,
                                                           const float *__restrict__ row_norm_max,
                                                           __half *__restrict__ qcast, float *__restrict__ qscale,
                                                           float *__restrict__ qeps, float *__restrict__ cscale,
                                                           float *__restrict__ ceps) {
    const int q = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (q >= nq) return;
    const int lane = threadIdx.x & (kWave - 1);
    const float *x = queries + (size_t)q * ld;
    __half *h = qcast + (size_t)q * ld16;
    const int nchunks = ld16 / 8;
    const bool in_regs = nchunks <= kWave * kCastChunks;  // (wavefront-uniform)
    CastChunk reg[kCastChunks];
    float m = 0.f;
    if (in_regs) {
#pragma unroll
        for (int j = 0; j < kCastChunks; j++) {
            const int c = lane + j * kWave;
            reg[j] = cast_chunk_load(x, c < nchunks ? c : nchunks, ld);  // (chunk nchunks: past the row, zeros, no load)
        }
#pragma unroll
        for (int j = 0; j < kCastChunks; j++) m = cast_chunk_max(reg[j], m);
    } else {
        for (int c = lane; c < nchunks; c += kWave) m = cast_chunk_max(cast_chunk_load(x, c, ld), m);
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float v = __shfl_xor(m, o);
        m = (v > m || v != v) ? v : m;
    }
    const int sq = scale_for(m);
    const double up = ldexp(1.0, sq);
    double qq4[4] = {0.0, 0.0, 0.0, 0.0}, dd4[4] = {0.0, 0.0, 0.0, 0.0}, hh4[4] = {0.0, 0.0, 0.0, 0.0};
    if (in_regs) {
#pragma unroll
        for (int j = 0; j < kCastChunks; j++) {
            const int c = lane + j * kWave;
            if (c < nchunks) cast_chunk_store(reg[j], c, ld, sq, up, h, qq4, dd4, hh4);
        }
    } else {
        for (int c = lane; c < nchunks; c += kWave) cast_chunk_store(cast_chunk_load(x, c, ld), c, ld, sq, up, h, qq4, dd4, hh4);
    }
    double qq = (qq4[0] + qq4[1]) + (qq4[2] + qq4[3]);  // |q|^2
    double dd = (dd4[0] + dd4[1]) + (dd4[2] + dd4[3]);  // |q - q^|^2
    double hh = (hh4[0] + hh4[1]) + (hh4[2] + hh4[3]);  // |q^|^2
    for (int o = 32; o > 0; o >>= 1) {
        qq += __shfl_xor(qq, o);
        dd += __shfl_xor(dd, o);
        hh += __shfl_xor(hh, o);
    }
    const double u = 5.9604644775390625e-8;
    if (lane == 0 && ceps) {
        // the center ranking: a = |c|^2 - 2^(1 + s_c + s_q) acc for s = |c|^2 - 2 q.c; |c|^2's own rounding is the
        // ScanBound's g_norm term, no pair term
        const int e = 1 + rt.s + sq;
        const double qn = sqrt(qq), dq = sqrt(dd), qh = sqrt(hh);
        const double cn = (double)*center_norm_max * (1.0 + rt.g_cn);
        double eps = 2.0 * (qn * rt.E + dq * rt.P)                       // representation of centers and query in fp16
                     + rt.g_dot * 2.0 * qh * rt.P                        // fp16 products, fp32 chains of the matrix cores
                     + 4.0 * u * (cn + 2.0 * qh * rt.P * (1.0 + rt.g_dot));  // epilogue: the final fmaf (|c|^2 + 0 is exact)
        eps = eps * (1.0 + 1.0 / 1048576.0) + 4.0 * (double)FLT_MIN;
        if (e < -125 || e > 125 || !(eps < 1e30)) eps = INFINITY;
        cscale[q] = ldexpf(1.f, e < -125 ? 0 : (e > 125 ? 0 : e));
        ceps[q] = (float)eps;
    }
    if (lane == 0 && qeps) {
        const int e = 1 + st.s + sq;
        const double qn = sqrt(qq), dq = sqrt(dd), qh = sqrt(hh);
        const double cmax = sqrt((double)*center_norm_max * (1.0 + st.g_cn)), rn = (double)*row_norm_max * (1.0 + st.g_cn);
        const double tmax = 2.0 * qn * cmax;  // |t| of every pair of this query (exact value)
        double eps = 2.0 * (qn * st.E + dq * st.P)               // representation of rows and query in fp16
                     + st.g_dot * 2.0 * qh * st.P                // fp16 products, fp32 chains of the matrix cores
                     + st.g_pair * tmax                          // the pair term's fp32 chain
                     + 4.0 * u * (rn + tmax * (1.0 + st.g_pair) + 2.0 * qh * st.P * (1.0 + st.g_dot));  // epilogue
        eps = eps * (1.0 + 1.0 / 1048576.0) + 4.0 * (double)FLT_MIN;  // fp32 rounding up; what underflowed on the way
        // a scale outside the normal fp32 range (or non-finite input) would not be exact: everything in the band
        if (e < -125 || e > 125 || !(eps < 1e30)) eps = INFINITY;
        qscale[q] = ldexpf(1.f, e < -125 ? 0 : (e > 125 ? 0 : e));
        qeps[q] = (float)eps;
    }
}

// One wavefront per probed (query, list) pair: t = -2 q.c_l into the pair's free word.  Each lane runs ONE fmaf chain
// over ceil(ld / 64) elements, then six shuffle additions: gamma_(ceil(ld / 64) + 6) |q||c_l| (ShadowTerms::g_pair,
// pair_chain_length).  For probe lists that did not come from this batch's own ranking (pgv_scan_batch, the sharded
// search): pgv_search_batch takes t from the ranking's exact recheck instead (batch_recheck_kernel, pair_t).
__global__ __launch_bounds__(256) void shadow_pair_kernel(const float *__restrict__ queries, const float *__restrict__ centers,
                                                          const int64_t *__restrict__ pair_start, int nlists, int64_t npairs,
                                                          int ld, ScanPair *__restrict__ pairs) {
    const int64_t pos = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pos >= npairs) return;
    const int lane = threadIdx.x & (kWave - 1);
    int lo = 0, hi = nlists - 1;  // last list whose first pair is <= pos
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pair_start[mid] <= pos)
            lo = mid;
        else
            hi = mid - 1;
    }
    const int q = pairs[pos].query;
    const float *x = queries + (size_t)q * ld;
    const float *c = centers + (size_t)lo * ld;
    float a = 0.f;
    for (int i = lane; i < ld; i += kWave) a = fmaf(x[i], c[i], a);
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if (lane == 0) pairs[pos].pad = (int32_t)__float_as_uint(-2.f * a);
}

}  // namespace

int launch_shadow_build(pgv_ctx *ctx, const RowGeom &g32, const RowGeom &g16, const void *rows, const void *centers,
                        const int64_t *list_off, int nlists, int64_t n, void *shadow, void *words, void *radius_bits) {
    if (n <= 0) return PGV_OK;
    // radius_bits (with centers; or null): [nlists] bits of the largest |x - c_l|^2 (fp64) of each list's rows
    if (radius_bits) PGV_HIP(hipMemsetAsync(radius_bits, 0, sizeof(unsigned long long) * (size_t)nlists, ctx->stream));
    // (centers null: the rows themselves are cast -- the shadow of an index's centers, E_c and P_c in the same words)
    // words: [0] max |rho_i| bits (u32) | [1..2] E^2, P^2 bits (u64 at byte 8)
    PGV_HIP(hipMemsetAsync(words, 0, 24, ctx->stream));
    unsigned *max_bits = static_cast<unsigned *>(words);
    unsigned long long *ep = reinterpret_cast<unsigned long long *>(static_cast<char *>(words) + 8);
    const dim3 grid((unsigned)((n + 3) / 4));
    hipLaunchKernelGGL(shadow_absmax_kernel, grid, dim3(256), 0, ctx->stream, static_cast<const float *>(rows),
                       static_cast<const float *>(centers), list_off, nlists, n, g32.ld, max_bits);
    hipLaunchKernelGGL(shadow_build_kernel, grid, dim3(256), 0, ctx->stream, static_cast<const float *>(rows),
                       static_cast<const float *>(centers), list_off, nlists, n, g32.ld, g16.ld, max_bits, static_cast<__half *>(shadow), ep,
                       centers ? static_cast<unsigned long long *>(radius_bits) : nullptr);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int shadow_scale_of(float max_abs) {
    if (!(max_abs > 0.f) || !std::isfinite(max_abs)) return 0;
    int e;
    (void)std::frexp(max_abs, &e);
    return e - 14;
}

int launch_shadow_query(pgv_ctx *ctx, const RowGeom &g32, const RowGeom &g16, const void *queries, int nq,
                        const ShadowTerms &st, const RankShadowTerms &rt, const float *center_norm_max,
                        const float *row_norm_max, void *qcast, float *qscale, float *qeps, float *cscale, float *ceps) {
    if (nq <= 0) return PGV_OK;
    hipLaunchKernelGGL(shadow_query_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, ctx->stream,
                       static_cast<const float *>(queries), nq, g32.ld, g16.ld, st, rt, center_norm_max, row_norm_max,
                       static_cast<__half *>(qcast), qscale, qeps, cscale, ceps);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_shadow_pairs(pgv_ctx *ctx, const RowGeom &g32, const void *queries, const void *centers,
                        const int64_t *pair_start, int nlists, int64_t npairs, ScanPair *pairs) {
    if (npairs <= 0) return PGV_OK;
    hipLaunchKernelGGL(shadow_pair_kernel, dim3((unsigned)((npairs + 3) / 4)), dim3(256), 0, ctx->stream,
                       static_cast<const float *>(queries), static_cast<const float *>(centers), pair_start, nlists, npairs,
                       g32.ld, pairs);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

}  // namespace pgv
