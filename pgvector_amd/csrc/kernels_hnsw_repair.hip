// kernels_hnsw_repair.hip -- hnswvacuum's repair search on the device: HnswFindElementNeighbors(..., existing = true)
// (src/hnswutils.c:1280-1357, called from RepairGraphElement, src/hnswvacuum.c:226-274) for a batch of linked elements of
// a dense mirror some of whose elements are dead (heaptidsLength == 0, pgv_hnsw_set_live), one workgroup per element.
//
// This is NOT the build's search (kernels_hnsw.hip).  With skipElement set, HnswSearchLayer counts only live elements
// towards ef (CountElement, src/hnswutils.c:715-728, used at :884 and :962):
//     alwaysAdd = wlen < ef; an element is admitted when alwaysAdd or eDistance < W's furthest      (:913, :936)
//     a LIVE admission raises wlen, which is never lowered, and once wlen > ef W's furthest is evicted, whatever kind
//         of entry that is                                                                          (:962-973)
//     a DEAD admission evicts nothing
// and the element itself, live on its page, is found and counted like any other -- which is why the caller's ef is
// ef_construction + 1 (:1316-1317).  Layers above the element's level are descended with ef = 1 under the same rule
// (:1306-1310 passes skipElement too).  After a layer's search W, nearest first, is stripped of the element itself and of
// the dead (RemoveElements, :1236-1259) and handed to SelectNeighbors (the existing device sweep: a plain sweep, no cached
// closer flags); the next layer's entry points are the UNSTRIPPED W (:1355).
//
// What the kernel has to get right:
//   * W grows past ef.  Every dead admission, and every live one while wlen < ef, adds an entry; a live admission with
//     wlen >= ef adds one and evicts one.  So |W| = |entry points| + (dead admitted) + (live admitted while wlen < ef) on
//     every layer, and the walk kernel's "stable merge truncated to ef" is wrong here.  Once wlen >= ef W's furthest key
//     never increases (an admission then needs a strictly smaller key, an eviction takes the furthest), so after a batch
//     of neighbours W is the first S entries of the stable merge of the admitted ones, S as above.  WHICH dead ones are
//     admitted depends on the order of admission inside the tuple (a dead element farther than a live one that follows it
//     is admitted only if it comes first), so that order is replayed: one wavefront walks the <= 2m scored neighbours in
//     tuple order, tests each against W's furthest and inserts it into the ONE ascending array that is W (wave-wide
//     rank by ballot, shift from the top down, 64 entries a step).
//   * The candidates are, as in the walk kernel, W's entries not yet expanded; an entry evicted at a key equal to W's new
//     furthest stays a candidate in the reference (its stop test is strict, :894) and goes to the tie list T.  T keeps its
//     meaning and its bound: when the first entry leaves W at K with K W's furthest key, wlen >= ef, nothing at K is
//     admitted from then on, so whatever enters T at K was in W at that moment and one of those stays: |T| < |W| <= wcap.
//   * Capacity.  W holds wcap = ef_construction + 1 + dead_cap entries in LDS.  An admission that would need one more
//     stops the element's search: out_status = 1, its counts stay 0, nothing is written past W.  It is never a shorter
//     list.  On ONE layer |W| <= max(|entry points|, ef) + (dead elements), so a single-layer graph cannot overflow a
//     dead_cap of the number of dead elements; across layers a dead element evicted on one layer can be admitted again
//     on the next while the live entry that replaced it is still among the entry points, so the certain bound is
//     (layers searched) x (dead elements) -- callers double dead_cap and redo (pgv_host_hnsw_repair).
//   * A separate kernel: hnsw_search_kernel's instantiations are not touched (profiles/r31_hnsw_repair.md has their
//     resource usage on both commits).  The row scoring is the walk's: the same loads, the same accumulator per row and
//     the same element order, so a distance is the walk's distance bit for bit.
#include "pgv_device.h"

namespace pgv {

namespace {

constexpr int kRepairThreads = 256;
constexpr int kRepairWaves = kRepairThreads / kWave;
constexpr uint32_t kRepairExpanded = 0x80000000u;
constexpr size_t kRepairScalarBytes = 64, kRepairLdsLimit = 150 * 1024;

struct RepairDev {
    const char *rows;  // [n x nvec] 16-byte vectors
    int nvec, lpr_log2, nchunks;
    const int32_t *levels;     // [n]
    const int64_t *nbr_start;  // [n + 1]
    const int32_t *nbr;        // neighbour tuples, HnswNeighborTupleData layout
    const uint32_t *live;      // element e: bit e & 31 of word e >> 5; NULL: every element is live
    int m;
    int32_t entry;
    int64_t n;
};

struct RepairRun {
    const int32_t *qids;  // [nq] the elements being repaired
    int nq, ef, wcap;     // ef = ef_construction + 1; W's capacity
    int32_t *lw_ids;      // [nq x lcap x wcap] the stripped W of every searched layer <= the element's level, nearest first
    float *lw_dist;       // [nq x lcap x wcap]
    int32_t *lw_cnt;      // [nq x lcap] (0 for layers not searched, and for every layer of an overflowed element)
    int32_t *qlevels;     // [nq] out: the element's level (what the selection kernels take as the insert level)
    int32_t *status;      // [nq] out: 1 = W overflowed its capacity
    int lcap;
};

struct RepairScalars {
    int query, wn, nb, cand;
    int wlen;       // live elements admitted to W on this layer, entry points included; never lowered
    int tn, tread;  // |T|; T's next unread entry
    uint32_t tkey;  // the key T's entries share
    int over;
};
static_assert(sizeof(RepairScalars) <= kRepairScalarBytes, "LDS region too small");

// The kernel's dynamic LDS, byte offsets:
//   query row | W keys [wcap] | W ids [wcap] | T ids [wcap] | batch keys [2 m] | batch ids [2 m] | batch flags [2 m] | scalars
struct RepairLds {
    size_t wk, wi, ti, bk, bi, bf, sc, total;
    __host__ __device__ constexpr RepairLds(size_t query_bytes, int wcap, int m)
        : wk(query_bytes), wi(wk + (size_t)wcap * 4), ti(wi + (size_t)wcap * 4), bk(ti + (size_t)wcap * 4),
          bi(bk + 2 * (size_t)m * 4), bf(bi + 2 * (size_t)m * 4), sc(bf + 2 * (size_t)m * 4), total(sc + kRepairScalarBytes) {}
};

__device__ __forceinline__ int repair_wave_append(bool take, int lane, int &count) {
    const unsigned long long bal = __ballot(take);
    const int at = count + __popcll(bal & ((1ull << lane) - 1ull));
    count += __popcll(bal);
    return at;
}

template <typename T, int METRIC>
__global__ __launch_bounds__(kRepairThreads) void hnsw_repair_kernel(RepairDev g, RepairRun run, uint32_t *__restrict__ bitmaps,
                                                                      int words, int *__restrict__ qcounter) {
    constexpr int N = VecTraits<T>::N;
    const int nq = run.nq, wcap = run.wcap;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lm0 = 2 * g.m;
    Raw16 *lq = reinterpret_cast<Raw16 *>(smem);
    const RepairLds at((size_t)g.nvec * sizeof(Raw16), wcap, g.m);
    uint32_t *wk = reinterpret_cast<uint32_t *>(smem + at.wk);
    uint32_t *wi = reinterpret_cast<uint32_t *>(smem + at.wi);
    uint32_t *ti = reinterpret_cast<uint32_t *>(smem + at.ti);
    uint32_t *bk = reinterpret_cast<uint32_t *>(smem + at.bk);
    int32_t *bi = reinterpret_cast<int32_t *>(smem + at.bi);
    uint32_t *bf = reinterpret_cast<uint32_t *>(smem + at.bf);  // bit 0: live; bit 1: on this layer (level >= lc)
    RepairScalars &sc = *reinterpret_cast<RepairScalars *>(smem + at.sc);

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lpr = 1 << g.lpr_log2;
    const int sub = lane & (lpr - 1);
    const int rsub = lane >> g.lpr_log2;
    const int rpw = kWave >> g.lpr_log2;
    const size_t row_bytes = (size_t)g.nvec * sizeof(Raw16);
    uint32_t *bitmap = bitmaps + (size_t)blockIdx.x * words;

    auto is_live = [&](uint32_t e) __attribute__((always_inline)) -> bool {
        return !g.live || ((g.live[e >> 5] >> (e & 31)) & 1u);
    };

    // distance of the query (in LDS) to the rows bi[0 .. nb) into bk: the walk's score_rows at four rows a trip -- every
    // row its own accumulator, the elements in the same order, so the keys are the walk's
    auto score_batch = [&](int nb) __attribute__((always_inline)) {
        constexpr int R = 4;
        const int step = kRepairWaves * rpw;
        for (int base = wave * rpw; base < nb; base += R * step) {
            int idx[R];
            bool valid[R];
            const char *rp[R];
            float acc[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                idx[r] = base + rsub + r * step;
                valid[r] = idx[r] < nb;
                rp[r] = g.rows + (size_t)bi[valid[r] ? idx[r] : nb - 1] * row_bytes;
                acc[r] = 0;
            }
#pragma unroll 2
            for (int c = 0; c < g.nchunks; c++) {
                const int vi = c * lpr + sub;
                const bool ok = vi < g.nvec;
                const int vc = ok ? vi : g.nvec - 1;  // never predicate a load
                Raw16 rv[R];
#pragma unroll
                for (int r = 0; r < R; r++) rv[r] = load16(rp[r] + (size_t)vc * sizeof(Raw16));
                const Raw16 qv = lq[vc];
                Unpacked<T> uq(qv);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    Unpacked<T> ur(rv[r]);
#pragma unroll
                    for (int e = 0; e < N; e++) acc[r] = accum<METRIC>(acc[r], ok ? ur.v[e] : 0.f, ok ? uq.v[e] : 0.f);
                }
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float sum = group_sum_to_last(acc[r], g.lpr_log2);
                if (sub == lpr - 1 && valid[r]) bk[idx[r]] = float_to_key(finish<METRIC>(sum));
            }
        }
    };

    // a fresh visited set holding the layer's entry points (src/hnswutils.c:862-886): the previous layer's unstripped W,
    // all unexpanded again; wlen counts the live ones
    auto enter_layer = [&]() __attribute__((always_inline)) {
        for (int w = tid; w < words; w += kRepairThreads) bitmap[w] = 0u;
        __syncthreads();
        const int wn = sc.wn;
        for (int j = tid; j < wn; j += kRepairThreads) {
            const uint32_t id = wi[j] & ~kRepairExpanded;
            wi[j] = id;
            atomicOr(&bitmap[id >> 5], 1u << (id & 31));
        }
        if (wave == 0) {
            int wlen = 0;
            for (int base = 0; base < wn; base += kWave) {
                const int j = base + lane;
                const uint32_t id = wi[j < wn ? j : wn - 1] & ~kRepairExpanded;  // never predicate a load
                wlen += __popcll(__ballot(j < wn && is_live(id)));
            }
            if (lane == 0) {
                sc.wlen = wlen;
                sc.tn = sc.tread = 0;
            }
        }
    };
    // wavefront 0: the next candidate -- W's first unexpanded entry, or with W exhausted an evicted one tied with its
    // furthest -- into sc.cand, and its unvisited neighbours at layer lc, in tuple order, into bi[0 .. sc.nb)
    auto next_candidate = [&](int lc, int lm) __attribute__((always_inline)) {
        const int wn = sc.wn;
        int found = -1;
        for (int base = 0; base < wn && found < 0; base += kWave) {
            const int j = base + lane;
            const bool open = j < wn && !(wi[j] & kRepairExpanded);
            const unsigned long long bal = __ballot(open);
            if (bal) found = base + __ffsll((long long)bal) - 1;
        }
        int nb = 0, cand = -1;
        if (found >= 0) {
            cand = (int)wi[found];
            if (lane == 0) wi[found] = (uint32_t)cand | kRepairExpanded;
        } else if (sc.tread < sc.tn) {
            cand = (int)ti[sc.tread];
            if (lane == 0) sc.tread = sc.tread + 1;
        }
        if (cand >= 0) {
            const uint32_t c = (uint32_t)cand;
            const int64_t start = g.nbr_start[c] + (int64_t)(g.levels[c] - lc) * g.m;  // (src/hnswutils.c:786)
            for (int base = 0; base < lm; base += kWave) {
                const int j = base + lane;
                const int32_t e = j < lm ? g.nbr[start + j] : -1;
                bool fresh = false;
                if (e >= 0 && e < g.n) {
                    const uint32_t bit = 1u << (e & 31);
                    fresh = !(atomicOr(&bitmap[e >> 5], bit) & bit);
                }
                const int slot = repair_wave_append(fresh, lane, nb);
                if (fresh) bi[slot] = e;
            }
        }
        if (lane == 0) {
            sc.nb = nb;
            sc.cand = cand;
        }
    };
    // wavefront 0: the scored batch admitted one by one, in tuple order (src/hnswutils.c:908-975) -- see the header
    auto admit_batch = [&](int lc, int ef_l, int nb) __attribute__((always_inline)) {
        for (int i = lane; i < nb; i += kWave) {
            const uint32_t e = (uint32_t)bi[i];
            bf[i] = (is_live(e) ? 1u : 0u) | ((lc == 0 || g.levels[e] >= lc) ? 2u : 0u);
        }
        int wn = sc.wn, wlen = sc.wlen, tn = sc.tn, tread = sc.tread;
        uint32_t tkey = sc.tkey;
        bool over = false;
        for (int i = 0; i < nb; i++) {
            const uint32_t key = __builtin_amdgcn_readfirstlane(bk[i]);
            const uint32_t flags = __builtin_amdgcn_readfirstlane(bf[i]);
            const uint32_t furthest = __builtin_amdgcn_readfirstlane(wk[wn - 1]);  // (wn >= 1: the entry points)
            if (!(wlen < ef_l || key < furthest)) continue;
            if (!(flags & 2u)) continue;  // "make robust to issues" (:947-949)
            bool evict = false;
            if (flags & 1u) {
                wlen++;
                evict = wlen > ef_l;
            }
            uint32_t ekey = 0, eid = 0;
            if (evict) {
                // (wlen was >= ef: the newcomer is strictly nearer than the furthest, which is the one that leaves)
                ekey = furthest;
                eid = __builtin_amdgcn_readfirstlane(wi[wn - 1]);
                wn--;
            } else if (wn >= wcap) {
                over = true;
                break;
            }
            // the newcomer goes behind every entry that is not farther
            int p = 0;
            for (int base = 0; base < wn; base += kWave) {
                const int j = base + lane;
                p += __popcll(__ballot(j < wn && wk[j < wn ? j : 0] <= key));
            }
            // entries [p, wn) move up by one, from the top down: a step reads its (at most 64) entries, then writes them
            for (int hi = wn; hi > p; hi -= kWave) {
                const int lo = hi - kWave > p ? hi - kWave : p;
                const int j = lo + lane;
                const bool mv = j < hi;
                const uint32_t mk = wk[mv ? j : lo], mi = wi[mv ? j : lo];
                if (mv) {
                    wk[j + 1] = mk;
                    wi[j + 1] = mi;
                }
            }
            if (lane == 0) {
                wk[p] = key;
                wi[p] = (uint32_t)bi[i];
            }
            wn++;
            if (evict) {
                const uint32_t K = __builtin_amdgcn_readfirstlane(wk[wn - 1]);
                if (tn > 0 && tkey != K) tn = tread = 0;
                if (ekey == K && !(eid & kRepairExpanded)) {
                    if (tn == 0) {
                        tkey = K;
                        tread = 0;
                    }
                    if (lane == 0 && tn < wcap) ti[tn] = eid;  // (tn < wcap always: the guard only keeps a write inside T)
                    if (tn < wcap) tn++;
                }
            }
        }
        if (lane == 0) {
            sc.wn = wn;
            sc.wlen = wlen;
            sc.tn = tn;
            sc.tread = tread;
            sc.tkey = tkey;
            if (over) sc.over = 1;
        }
    };
    // wavefront 0: layer lc's W without the element itself and without the dead, nearest first: what SelectNeighbors sees
    auto hand_out_w = [&](int qi, int lc, uint32_t self) __attribute__((always_inline)) {
        const int wn = sc.wn;
        const size_t o = ((size_t)qi * run.lcap + lc) * wcap;
        int out = 0;
        for (int base = 0; base < wn; base += kWave) {
            const int j = base + lane < wn ? base + lane : wn - 1;  // never predicate a load
            const uint32_t id = wi[j] & ~kRepairExpanded, key = wk[j];
            const bool keep = base + lane < wn && id != self && is_live(id);
            const int slot = repair_wave_append(keep, lane, out);
            if (keep) {  // (slot < wn <= wcap)
                run.lw_ids[o + slot] = (int32_t)id;
                run.lw_dist[o + slot] = key_to_float(key);
            }
        }
        if (lane == 0) run.lw_cnt[(size_t)qi * run.lcap + lc] = out;
    };

    for (;;) {
        if (tid == 0) sc.query = atomicAdd(qcounter, 1);
        __syncthreads();
        const int qi = sc.query;
        if (qi >= nq) return;
        const int32_t self = run.qids[qi];
        const bool known = self >= 0 && self < g.n;  // (a slot outside the mirror is searched for nothing: counts 0)
        const int level = g.levels[known ? self : 0];
        for (int l = tid; l < run.lcap; l += kRepairThreads) run.lw_cnt[(size_t)qi * run.lcap + l] = 0;
        if (tid == 0) {
            run.status[qi] = 0;
            run.qlevels[qi] = level;
            sc.over = 0;
        }
        if (g.entry < 0 || !known) {  // no entry point: no neighbors (:1297-1299)
            __syncthreads();
            continue;
        }
        {
            const char *qrow = g.rows + (size_t)self * row_bytes;
            for (int v = tid; v < g.nvec; v += kRepairThreads) lq[v] = load16(qrow + (size_t)v * sizeof(Raw16));
        }
        if (tid == 0) bi[0] = g.entry;
        __syncthreads();
        score_batch(1);
        __syncthreads();
        if (tid == 0) {
            wk[0] = bk[0];
            wi[0] = (uint32_t)g.entry;
            sc.wn = 1;
        }
        bool over = false;
        for (int lc = g.levels[g.entry]; lc >= 0 && !over; lc--) {
            const int ef_l = lc <= level ? run.ef : 1;
            const int lm = lc == 0 ? lm0 : g.m;
            __syncthreads();
            enter_layer();
            __syncthreads();
            for (;;) {
                if (wave == 0) next_candidate(lc, lm);
                __syncthreads();
                const int nb = sc.nb;
                if (sc.cand < 0) break;
                if (nb == 0) {
                    __syncthreads();
                    continue;
                }
                score_batch(nb);
                __syncthreads();
                if (wave == 0) admit_batch(lc, ef_l, nb);
                __syncthreads();
                if (sc.over) {
                    over = true;
                    break;
                }
            }
            __syncthreads();
            if (!over && lc <= level && lc < run.lcap && wave == 0) hand_out_w(qi, lc, (uint32_t)self);
        }
        __syncthreads();
        if (over) {
            for (int l = tid; l < run.lcap; l += kRepairThreads) run.lw_cnt[(size_t)qi * run.lcap + l] = 0;
            if (tid == 0) run.status[qi] = 1;
        }
        __syncthreads();
    }
}

}  // namespace

size_t hnsw_repair_lds_bytes(const RowGeom &geom, int ef_construction, int dead_cap, int m) {
    return RepairLds((size_t)geom.nvec * sizeof(Raw16), ef_construction + 1 + dead_cap, m).total;
}

int hnsw_repair_dead_cap_max(const RowGeom &geom, int ef_construction, int m) {
    const size_t base = hnsw_repair_lds_bytes(geom, ef_construction, 0, m);
    if (base > kRepairLdsLimit) return -1;
    const size_t room = (kRepairLdsLimit - base) / 12;
    return room > 0x3fffffff ? 0x3fffffff : (int)room;
}

int hnsw_repair_lds_check(const char *who, const RowGeom &geom, int ef_construction, int dead_cap, int m, size_t *lds_out) {
    const size_t lds = hnsw_repair_lds_bytes(geom, ef_construction, dead_cap, m);
    if (lds_out) *lds_out = lds;
    if (lds > kRepairLdsLimit)
        PGV_FAIL(PGV_ERR_ARG, "%s: ef %d / dead_cap %d / m %d need %zu bytes of LDS (limit %d)", who, ef_construction + 1, dead_cap,
                 m, lds, (int)kRepairLdsLimit);
    return PGV_OK;
}

int launch_hnsw_repair(pgv_ctx *ctx, const RowsView &v, const HnswGraph &graph, const uint32_t *live, const HnswRepairArgs &a,
                       uint32_t *bitmaps, int words, int grid, int *counter) {
    if (v.bits() || v.sparse()) PGV_FAIL(PGV_ERR_ARG, "hnsw repair: dense rows only");
    size_t lds = 0;
    PGV_TRY(hnsw_repair_lds_check("hnsw repair", v.geom, a.ef_construction, a.dead_cap, graph.m, &lds));
    RepairDev g;
    g.rows = static_cast<const char *>(v.rows);
    g.nvec = v.geom.nvec;
    g.lpr_log2 = v.geom.lpr_log2;
    g.nchunks = v.geom.nchunks;
    g.levels = graph.levels;
    g.nbr_start = graph.nbr_start;
    g.nbr = graph.nbr;
    g.live = live;
    g.m = graph.m;
    g.entry = graph.entry;
    g.n = v.n;
    RepairRun run;
    run.qids = a.qids;
    run.nq = a.nq;
    run.ef = a.ef_construction + 1;
    run.wcap = a.ef_construction + 1 + a.dead_cap;
    run.lw_ids = a.lw_ids;
    run.lw_dist = a.lw_dist;
    run.lw_cnt = a.lw_cnt;
    run.qlevels = a.qlevels;
    run.status = a.status;
    run.lcap = a.lcap;
    PGV_HIP(hipMemsetAsync(counter, 0, sizeof(int), ctx->stream));
    return dispatch_metric(v.metric, v.dtype(), [&](auto *tp, auto mc) {
        auto kern = hnsw_repair_kernel<std::remove_pointer_t<decltype(tp)>, decltype(mc)::value>;
        PGV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kRepairThreads), lds, ctx->stream, g, run, bitmaps, words, counter);
        PGV_HIP(hipGetLastError());
        return PGV_OK;
    });
}

}  // namespace pgv
