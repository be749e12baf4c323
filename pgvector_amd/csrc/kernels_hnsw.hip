// kernels_hnsw.hip -- hnswgettuple's first batch entirely on the device: the greedy
// descent through the upper layers and HnswSearchLayer on layer 0
// (src/hnswscan.c:25-56, src/hnswutils.c:824-987), one workgroup per query.
//
// The reference keeps two pairing heaps per layer search: C, the candidates still to
// expand (nearest first), and W, the ef nearest elements found (furthest first).
// Every element enters both at once (:936-960); W evicts its furthest when it
// overflows (:967-973); the search stops when the nearest unexpanded candidate is
// strictly farther than W's furthest (:894).  A candidate that has been evicted from
// W is at least as far as W's furthest from then on, so it can never be expanded
// before the search stops: C is, for the purposes of the result, "the entries of W
// not expanded yet".  Here W is therefore ONE ascending array in LDS whose entries
// carry an `expanded` flag:
//   next candidate  = first unexpanded entry (none left <=> the reference's loop ends)
//   neighbours      = the candidate's neighbour tuple at this layer, in tuple order,
//                     minus the visited ones (visited set: a bitmap in HBM)
//   scoring         = all unvisited neighbours at once, every wavefront of the
//                     workgroup taking rows (the distances do not depend on heap state)
//   admission       = a stable merge of the scored batch into W truncated to ef, which
//                     is exactly what admitting them one by one with the reference's
//                     `eDistance < f->distance || wlen < ef` test produces: an element
//                     rejected or evicted on the way would sit past position ef in
//                     the merged order as well.
// One refinement keeps this exact for distance ties: an element that was admitted and
// then evicted from W at a distance EQUAL to W's new furthest is still a live
// candidate in the reference (its stop test is strict).  Such elements go to a
// tie list T (they all share one distance); T is dropped as soon as W's furthest
// gets nearer, and its members are expanded after W's own unexpanded entries.  The
// ORDER among equal distances is the one thing left open -- it is unspecified in the
// reference as well (pairing-heap internals).
// T has ef slots and never fills them.  When the first entry leaves W at K while K is
// W's furthest key, W is full of keys <= K, and from then on nothing at K is admitted
// (`eDistance < f->distance` fails).  So everything that ever enters T at K was among
// the at most ef entries not farther than K at that moment -- W's old entries
// and the batch entries admitted in their turn -- and at least one of those stays in
// W for K to remain its furthest key: |T| <= ef - 1.  (tests/hnsw_walk_model.py
// asserts the bound on every batch of every walk it models.)
//
// A resumable scan (pgv_hnsw_scan_*, hnsw.iterative_scan) is the same kernel with SCAN = true: the visited bitmap belongs
// to the query, what the merge leaves past position ef goes to a per-query pool, and a later batch starts layer 0 from
// the pool's nearest entries (ResumeScanItems, src/hnswscan.c:61-87) -- see HnswScanDev and scan_entry_step.
//
// Keys are uint32 throughout and only ever compared.  fp32 and fp16 mirrors, Hamming bit mirrors and sparse mirrors rank by
// float_to_key of an fp32 distance that is the reference's float8 exactly; a Jaccard bit mirror (<BitRow, 1>,
// pgv_hnsw_upload_jaccard) ranks by jaccard_key, an integer image of the ratio that orders and ties as its float8 does.
#include "pgv_device.h"
#include "sparse_pair.h"

#include <type_traits>

#include <cstdlib>

namespace pgv {

namespace {

constexpr int kHnswThreads = 256;
constexpr int kHnswWaves = kHnswThreads / kWave;
constexpr uint32_t kExpanded = 0x80000000u;

struct HnswDev {
    const char *rows;  // [n x nvec] 16-byte vectors; a sparse mirror: the rows' (index, value) pairs, row after row
    int nvec, lpr_log2, nchunks;
    const int32_t *levels;     // [n]
    const int64_t *nbr_start;  // [n + 1]
    const int32_t *nbr;        // neighbour tuples, HnswNeighborTupleData layout
    int m;
    int32_t entry;
    int64_t n;
};

// One launch's queries and outputs.  A scan passes query vectors and wants the k nearest of
// layer 0.  The build (HnswFindElementNeighbors, src/hnswutils.c:1280-1357) passes element slots
// as queries plus each element's insert level: layers above it are descended greedily (ef = 1),
// layers at or below it are searched with ef_construction and their whole W is returned.
struct HnswRun {
    const char *queries;      // [nq x nvec] 16-byte vectors, or NULL with qids
    const int32_t *qids;      // query i = element qids[i] of the mirror (build), or NULL
    const int32_t *qlevels;   // insert level per query (build), or NULL = 0
    int nq, ef, k;
    int64_t *out_elem;        // [nq x k] or NULL
    float *out_dist;          // [nq x k] or NULL
    int64_t *out_scored;      // [nq] or NULL
    int32_t *lw_ids;          // [nq x lcap x ef] W of every searched layer <= the insert level, nearest first; or NULL
    float *lw_dist;           // [nq x lcap x ef]
    int32_t *lw_cnt;          // [nq x lcap] |W| (0 for layers not searched)
    int lcap;
    int rows_per_trip;        // rows a lane group scores at once: 1, 2 or 4 (PGV_HNSW_ROWS_PER_TRIP, for A/B runs)
};

// What a walk over sparse rows takes on top (the kernel's LAST argument, so that the other kinds' arguments stay where they
// were): where each row's pairs start, the queries in CSR, the pairs the LDS query region holds (the batch's longest
// query, padded), the words of one wavefront's matched bitmap (0: inner product) and whether a wavefront fetches its next
// row while it searches the current one (PGV_HNSW_SPARSE_PREFETCH, for A/B runs)
struct HnswSparse {
    const int64_t *row_ptr;  // [n + 1]
    const int64_t *q_ptr;    // the queries in CSR; NULL with run.qids (the build: query i is element qids[i], read at row_ptr)
    const int32_t *q_idx;
    const float *q_val;
    int q_cap, bm_words, prefetch;
};

// bytes of the query region of a sparse walk's LDS: the query's pairs, then one matched bitmap per wavefront
__host__ __device__ inline size_t sparse_query_bytes(int sq_cap, int bm_words) {
    return (size_t)sq_cap * sizeof(QElem) + (size_t)kHnswWaves * bm_words * sizeof(uint32_t);
}

// What a resumable scan (pgv_hnsw_scan_*, SCAN = true) over dense or bit rows takes in the place of HnswSparse: the last
// argument is one or the other, and the plain walks' arguments stay where they were (a scan over sparse rows takes both,
// HnswSparseScan below).  Per query: its visited bitmap (bitmaps[q * words ..), never shared between workgroups), the pool
// of discarded candidates in the order they were discarded ((key, element) pairs, pool[q * cap ..)), and HnswScanQuery.  A
// query is one workgroup's for a whole launch.
struct HnswScanQuery {
    int64_t tuples;   // so->tuples so far
    int32_t pool_n;   // live pool entries
    int32_t flags;    // kScanStarted | kScanOverflow
};
constexpr int kScanStarted = 1, kScanOverflow = 2;
static_assert(sizeof(HnswScanQuery) == kHnswScanQueryBytes, "the host sizes a scan's per-query state by kHnswScanQueryBytes");
struct HnswScanDev {
    uint2 *pool;
    int cap;                // pool entries per query
    HnswScanQuery *qs;      // [nq]
    const uint8_t *want;    // [nq] or NULL = every query
    int32_t *out_count;     // [nq]
    int64_t *out_left;      // [nq] or NULL
    int *overflow;          // 0, or 1 + the first query seen to overflow its pool
    int drain;              // pgv_hnsw_scan_drain: the entry step alone
};
// ... and a scan over sparse rows (pgv_hnsw_scan_begin_sparse, <SparseRow, METRIC, SCAN = true>): the scan's state and the
// sparse walk's extras in one last argument, of this form only -- every other instantiation keeps the argument it had.
// q_ptr / q_idx / q_val are the scan's own copy of its queries; q_cap / bm_words come from the SCAN's longest query,
// whichever queries a launch wants
struct HnswSparseScan : HnswScanDev {
    HnswSparse sp;
};
// ... and a filtered scan (pgv_hnsw_scan_filtered, FILTER = true) on top of either: hnswgettuple's loop
// (src/hnswscan.c:242-327) for one query inside one workgroup.  run.k is then the width of the output rows, run.ef the
// scan's batch size.  Forms of their own again: every other instantiation keeps the argument it had.
template <typename Base>
struct HnswFiltered : Base {
    const uint32_t *keep;  // element e: bit e & 31 of word e >> 5; NULL keeps everything
    int64_t keep_stride;   // words between two queries' bitmaps; 0: one bitmap for all
    int64_t max_tuples;    // hnsw.max_scan_tuples: from so->tuples >= this on the pool is drained, not walked
    int strict;            // strict_order: an element nearer than the last one that passed is dropped
    int32_t *out_batches;  // [nq] or NULL: walks plus drains taken
};
template <typename L> constexpr bool kIsFiltered = false;
template <typename B> constexpr bool kIsFiltered<HnswFiltered<B>> = true;

// A walk's scalars in LDS, one workgroup's
struct WalkScalars {
    int query, wn, nb;  // the query being walked; |W|; the size of the batch being scored
    int cand, cur;      // the candidate being expanded (-1: none left); which of W's two buffers is live
    int tn, tread;      // |T|; T's next unread entry
    uint32_t tkey;      // the key T's entries share
    int pool_n;         // a scan's live pool entries, for the batch
    // a filtered scan's query (FILTER): the rows its last batch emitted, the last key that passed strict_order, walks plus
    // drains taken (the rows emitted so far are a register of every thread: see filter_batch)
    int got;
    uint32_t prev;
    int batches;
};
// what a scan's entry step keeps in LDS on top: the radix descent's histogram, its verdict, and each wavefront's counts
struct ScanEntryLds {
    uint32_t hist[256];
    int bucket, rank;  // the pass's digit and the rank left inside it
    int lt[kHnswWaves], eq[kHnswWaves];
};
constexpr size_t kWalkScalarBytes = 64, kScanEntryBytes = (256 + 16) * sizeof(uint32_t), kHnswLdsLimit = 150 * 1024;
static_assert(sizeof(WalkScalars) <= kWalkScalarBytes && sizeof(ScanEntryLds) <= kScanEntryBytes, "LDS regions too small");

// The walk's dynamic LDS, byte offsets (the query region starts at 0): what the launcher sizes and the kernel carves.
//   query row | W keys [2][ef] | W ids [2][ef] | batch keys [2 m] | batch ids [2 m] | T ids [ef] | WalkScalars | ScanEntryLds
// (a sparse walk's query region: the query's (index, value) pairs [sq_cap] | matched bitmaps [waves][bm_words])
struct HnswLds {
    size_t wk, wi, bk, bi, ti, sc, entry, total;
    __host__ __device__ constexpr HnswLds(size_t query_bytes, int ef, int m, bool scan)
        : wk(query_bytes), wi(wk + 2 * (size_t)ef * 4), bk(wi + 2 * (size_t)ef * 4), bi(bk + 2 * (size_t)m * 4),
          ti(bi + 2 * (size_t)m * 4), sc(ti + (size_t)ef * 4), entry(sc + kWalkScalarBytes),
          total(entry + (scan ? kScanEntryBytes : 0)) {}
};
static_assert(HnswLds(6144, 1000, 100, false).total == 6144 + 1000 * 16 + 100 * 16 + 1000 * 4 + 64 &&
                  HnswLds(16, 1, 2, true).total == 16 + 16 + 32 + 4 + 64 + 1088,
              "a walk takes query_bytes + ef * 16 + m * 16 + ef * 4 + 64 bytes of LDS, a scan 1088 more");

// Wavefront compaction: the lanes whose `take` holds get consecutive slots from `count` on, in lane order.  Returns this
// lane's slot (to be used where take holds; the caller guards its store) and moves count past the takers.  A whole
// wavefront calls.
__device__ __forceinline__ int wave_append(bool take, int lane, int &count) {
    const unsigned long long bal = __ballot(take);
    const int at = count + __popcll(bal & ((1ull << lane) - 1ull));
    count += __popcll(bal);
    return at;
}

// Where the stable merge of a scored batch (keys bk[0 .. nb), batch order) into W (keys ck[0 .. wn), ascending) puts an
// entry.  The new W, the tie list and a scan's pool all ask here: |T| <= ef - 1 and the pool's discard order rest on
// their agreeing.
struct MergePos {
    const uint32_t *ck, *bk;
    int wn, nb;
    // old entry j (key = ck[j]) moves up by the batch entries strictly nearer
    __device__ __forceinline__ int old_slot(int j, uint32_t key) const {
        int s = j;
        for (int b = 0; b < nb; b++) s += bk[b] < key;
        return s;
    }
    // batch entry i (key = bk[i]) goes after every old entry that is not farther and after the batch entries that are
    // nearer or equal-and-earlier.  T's own quantity comes out of the same pass: `before`, the entries not farther
    // that are there when its turn comes -- those old entries, and the batch entries ahead of it.
    __device__ __forceinline__ int batch_slot(int i, uint32_t key, int &before) const {
        int lo = 0, hi = wn;  // first old entry with key > this one
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ck[mid] <= key)
                lo = mid + 1;
            else
                hi = mid;
        }
        int s = lo;
        before = lo;
        for (int b = 0; b < nb; b++) {
            before += b < i && bk[b] <= key;
            s += (bk[b] < key) || (bk[b] == key && b < i);
        }
        return s;
    }
    __device__ __forceinline__ int batch_slot(int i, uint32_t key) const { int unused; return batch_slot(i, key, unused); }
};

// The entry step of a resumed batch (ResumeScanItems' pairingheap_remove_first loop, src/hnswscan.c:61-87, in bulk): the
// `take` smallest of pool[0 .. pn) by (key, position) into wk0 / wi0 in that order; the rest of the pool closes up, order
// kept.  stage_k / stage_i: room for `take` entries (W's other buffer).  256 threads, all of them call.
//   1. the take-th smallest key K by an 8-bit radix descent over the keys (four passes over the pool), and how many of
//      the entries at exactly K are taken: the first `need` of them by position;
//   2. one pass in chunks of 256: a chunk is read into registers, __syncthreads(), then its taken entries go to the
//      stage in position order and its others back into the pool at or below the chunk's own reads;
//   3. rank-by-counting of the <= 1000 staged entries by (key, stage position) -- stage order is pool order.
__device__ __forceinline__ void scan_entry_step(uint2 *__restrict__ pool, int pn, int take, uint32_t *wk0, uint32_t *wi0,
                                                uint32_t *stage_k, uint32_t *stage_i, ScanEntryLds &el) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    uint32_t K = 0xffffffffu;
    int need = pn;  // pn <= take: everything goes, whatever its key
    if (pn > take) {
        uint32_t prefix = 0, mask = 0;
        int r = take;  // the r-th smallest of the keys that match prefix under mask
        for (int shift = 24; shift >= 0; shift -= 8) {
            el.hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < pn; i += kHnswThreads) {
                const uint32_t key = pool[i].x;
                if ((key & mask) == prefix) atomicAdd(&el.hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int acc = 0, b = 0;
                for (; b < 255; b++) {
                    const int c = (int)el.hist[b];
                    if (acc + c >= r) break;
                    acc += c;
                }
                el.bucket = b;
                el.rank = r - acc;
            }
            __syncthreads();
            prefix |= (uint32_t)el.bucket << shift;
            mask |= 255u << shift;
            r = el.rank;
            __syncthreads();
        }
        K = prefix;
        need = r;
    }
    int lt_run = 0, eq_run = 0;
    for (int base = 0; base < pn; base += kHnswThreads) {
        const int i = base + tid;
        const bool valid = i < pn;
        const uint2 e = pool[valid ? i : pn - 1];  // never predicate a load
        const bool is_lt = valid && e.x < K, is_eq = valid && e.x == K;
        int lt_mine = 0, eq_mine = 0;  // this wavefront's counts; the chunk's come from LDS
        int lt_before = lt_run + wave_append(is_lt, lane, lt_mine);
        int eq_before = eq_run + wave_append(is_eq, lane, eq_mine);
        if (lane == 0) {
            el.lt[wave] = lt_mine;
            el.eq[wave] = eq_mine;
        }
        __syncthreads();  // (the whole chunk is in registers from here on)
        for (int w = 0; w < kHnswWaves; w++) {
            const int l = el.lt[w], q = el.eq[w];
            if (w < wave) {
                lt_before += l;
                eq_before += q;
            }
            lt_run += l;
            eq_run += q;
        }
        const int sel_before = lt_before + (eq_before < need ? eq_before : need);
        const bool sel = is_lt || (is_eq && eq_before < need);
        if (sel) {
            if (sel_before < take) {  // (always: fewer than take entries are nearer than K, need of them at K)
                stage_k[sel_before] = e.x;
                stage_i[sel_before] = e.y;
            }
        } else if (valid) {
            pool[i - sel_before] = e;
        }
        __syncthreads();
    }
    for (int i = tid; i < take; i += kHnswThreads) {
        const uint32_t key = stage_k[i];
        int rank = 0;
        for (int j = 0; j < take; j++) rank += (stage_k[j] < key) || (stage_k[j] == key && j < i);
        wk0[rank] = key;
        wi0[rank] = stage_i[i];
    }
    __syncthreads();
}

__host__ __device__ __forceinline__ const HnswSparse &sparse_extras(const HnswSparse &sp, const HnswSparse &) { return sp; }
__host__ __device__ __forceinline__ const HnswSparse &sparse_extras(const HnswScanDev &, const HnswSparse &none) { return none; }
__host__ __device__ __forceinline__ const HnswSparse &sparse_extras(const HnswSparseScan &s, const HnswSparse &) { return s.sp; }

// the kernel's last argument: a sparse walk's extras, a scan's state, or -- a scan over sparse rows -- both; a filtered
// scan's wraps the scan's
template <typename T, bool SCAN>
using HnswLastPlain = std::conditional_t<SCAN, std::conditional_t<std::is_same_v<T, SparseRow>, HnswSparseScan, HnswScanDev>, HnswSparse>;
template <typename T, bool SCAN, bool FILTER = false>
using HnswLast = std::conditional_t<FILTER, HnswFiltered<HnswLastPlain<T, SCAN>>, HnswLastPlain<T, SCAN>>;

// ELEMQ (sparse rows only): the queries are element slots of the mirror, the build's form of a sparse walk.  An
// instantiation of its own, so that the plain sparse walks compile to what they were
// FILTER (with SCAN only): a query stays with its workgroup batch after batch -- walk or drain, filter, emit -- until it
// has its k rows, is exhausted or overflows (pgv_hnsw_scan_filtered); see the query loop below
template <typename T, int METRIC, bool SCAN = false, bool ELEMQ = false, bool FILTER = false>
__global__ __launch_bounds__(kHnswThreads) void hnsw_search_kernel(
    HnswDev g, HnswRun run, uint32_t *__restrict__ bitmaps, int words, int *__restrict__ qcounter,
    HnswLast<T, SCAN, FILTER> last) {
    static_assert(!FILTER || (SCAN && !ELEMQ), "a filtered scan is a scan");
    const HnswSparse none{};
    const HnswSparse &sp = sparse_extras(last, none);  // a sparse walk's extras (a dense or bit scan has none)
    const auto &ss = last;                             // a resumable scan's state (SCAN)
    const int nq = run.nq, ef = run.ef, k = run.k;
    int64_t *__restrict__ out_elem = run.out_elem;
    float *__restrict__ out_dist = run.out_dist;
    int64_t *__restrict__ out_scored = run.out_scored;
    constexpr int N = VecTraits<T>::N;
    constexpr bool kBits = std::is_same_v<T, BitRow>;
    constexpr bool kJaccard = kBits && METRIC == 1;  // bit_jaccard_ops: see score_rows
    constexpr bool kSparse = std::is_same_v<T, SparseRow>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lm0 = 2 * g.m;
    Raw16 *lq = reinterpret_cast<Raw16 *>(smem);
    const HnswLds at(kSparse ? sparse_query_bytes(sp.q_cap, sp.bm_words) : (size_t)g.nvec * sizeof(Raw16), ef, g.m, SCAN);
    uint32_t *wk = reinterpret_cast<uint32_t *>(smem + at.wk);
    uint32_t *wi = reinterpret_cast<uint32_t *>(smem + at.wi);
    uint32_t *bk = reinterpret_cast<uint32_t *>(smem + at.bk);
    int32_t *bi = reinterpret_cast<int32_t *>(smem + at.bi);
    uint32_t *ti = reinterpret_cast<uint32_t *>(smem + at.ti);  // tie list ids [ef]: |T| < ef, see the header
    WalkScalars &sc = *reinterpret_cast<WalkScalars *>(smem + at.sc);

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lpr = 1 << g.lpr_log2;
    const int sub = lane & (lpr - 1);
    const int rsub = lane >> g.lpr_log2;
    const int rpw = kWave >> g.lpr_log2;
    const size_t row_bytes = (size_t)g.nvec * sizeof(Raw16);
    uint32_t *bitmap = bitmaps + (size_t)blockIdx.x * words;  // (a scan's: the query's own, set below)

    // distance of the query (in LDS) to the rows bi[0 .. nb): every wavefront takes R x rpw rows per trip -- R rows' loads
    // in flight per lane group.  A walk is a chain of ~100 such batches, each waiting for its rows: with one row per trip
    // a batch of 32 neighbors was eight dependent round trips to HBM per wavefront (same box, 400 k x 1536, ef 100:
    // 352 k QPS with R = 1, 456 k with R = 2; 1 M x 1536: 366-403 k with R = 2, 385-413 k with R = 4, the default;
    // profiles/r05/hnsw_build_device_link.md).  Each row keeps its own accumulator and element order: the distances do not
    // depend on R.
    // A bit mirror (T = BitRow, bit_hamming_ops: hamming_distance, src/bitvec.c:45-56) counts the differing bits of the
    // same 16-byte vectors in an integer; the count (<= 64 000) and every partial sum of the reduction are exact in fp32.
    // A Jaccard mirror (<BitRow, 1>, bit_jaccard_ops: jaccard_distance, src/bitvec.c:60-70 over BitJaccardDistanceDefault,
    // src/bitutils.c:99-131) counts two integers in the same loop, x = popcount(a ^ b) and u = popcount(a | b), both exact
    // like the Hamming count, and one lane forms jaccard_key(x, u): an integer that orders and ties exactly as the
    // reference's float8 does (pgv_device.h), so everything that compares keys serves it unchanged.  A key does not carry
    // (x, u): where distances are handed back (OUT: a search's results, a build's W of every searched layer), the elements
    // jids[0 .. nb) -- at most ef -- are scored once more by this loop and jout[i] = jaccard_value(x, u), the (float) of the
    // reference's float8.
    const uint32_t *jids = nullptr;
    float *jout = nullptr;
    auto score_rows = [&](auto rc, auto oc, int nb) __attribute__((always_inline)) {
        constexpr int R = decltype(rc)::value;
        constexpr bool OUT = decltype(oc)::value;
        static_assert(!OUT || kJaccard, "only a Jaccard walk scores its results again");
        const int step = kHnswWaves * rpw;
        for (int base = wave * rpw; base < nb; base += R * step) {
            int idx[R];
            bool valid[R];
            const char *rp[R];
            std::conditional_t<kBits, int, float> acc[R];
            [[maybe_unused]] int uni[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                idx[r] = base + rsub + r * step;
                valid[r] = idx[r] < nb;
                if constexpr (OUT)
                    rp[r] = g.rows + (size_t)(jids[valid[r] ? idx[r] : nb - 1] & ~kExpanded) * row_bytes;
                else
                    rp[r] = g.rows + (size_t)bi[valid[r] ? idx[r] : nb - 1] * row_bytes;
                acc[r] = 0;
                if constexpr (kJaccard) uni[r] = 0;
            }
#pragma unroll 2
            for (int c = 0; c < g.nchunks; c++) {
                const int vi = c * lpr + sub;
                const bool ok = vi < g.nvec;
                const int vc = ok ? vi : g.nvec - 1;  // never predicate a load (see scan_kernel)
                Raw16 rv[R];
#pragma unroll
                for (int r = 0; r < R; r++) rv[r] = load16(rp[r] + (size_t)vc * sizeof(Raw16));
                const Raw16 qv = lq[vc];
                if constexpr (kJaccard) {
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        acc[r] += ok ? hamming16(rv[r], qv) : 0;
                        uni[r] += ok ? union16(rv[r], qv) : 0;
                    }
                } else if constexpr (kBits) {
#pragma unroll
                    for (int r = 0; r < R; r++) acc[r] += ok ? hamming16(rv[r], qv) : 0;
                } else if constexpr (!kSparse) {  // (a sparse walk never comes here: score_sparse below)
                    Unpacked<T> uq(qv);
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        Unpacked<T> ur(rv[r]);
#pragma unroll
                        for (int e = 0; e < N; e++) acc[r] = accum<METRIC>(acc[r], ok ? ur.v[e] : 0.f, ok ? uq.v[e] : 0.f);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float sum = group_sum_to_last((float)acc[r], g.lpr_log2);
                if constexpr (kJaccard) {
                    const int x = (int)sum, u = (int)group_sum_to_last((float)uni[r], g.lpr_log2);
                    if (sub == lpr - 1 && valid[r]) {
                        if constexpr (OUT)
                            jout[idx[r]] = jaccard_value(x, u);
                        else
                            bk[idx[r]] = jaccard_key(x, u);
                    }
                } else {
                    if (sub == lpr - 1 && valid[r]) bk[idx[r]] = float_to_key(finish<METRIC>(sum));
                }
            }
        }
    };
    // the distances of a Jaccard walk's results ids[0 .. cnt) into dst[0 .. cnt); the query is in LDS
    auto jaccard_out = [&](const uint32_t *ids, int cnt, float *dst) __attribute__((always_inline)) {
        if constexpr (kJaccard) {
            jids = ids;
            jout = dst;
            score_rows(std::integral_constant<int, 4>{}, std::true_type{}, cnt);
        }
    };
    // A sparse mirror (T = SparseRow; hnsw_sparsevec_support, src/hnswutils.c:1361-1433: FUNCTION 1 is
    // sparsevec_l2_squared_distance / _negative_inner_product / _l1_distance, src/sparsevec.c:826-869, :905-966, :1018-1060)
    // scores a whole row per wavefront with sparse_pair.h's score_element -- pgv_sparse_distance_batch's value for the pair,
    // bit for bit -- against the query's pairs in LDS.  Wavefront w takes rows w, w + 4, .. of the batch (at most 2 m / 4 <=
    // 50).  A batch is a dependent chain bi[] -> the row's bounds -> the row's pairs: lane j first loads the bounds of the
    // wavefront's j-th row, all rows at once, and with PREFETCH the pairs of the next row are requested before the current
    // one is searched (rows of up to 256 pairs: the register copy; a longer row is read inside its search).
    int sqn = 0;  // the current query's stored elements
    auto score_sparse = [&](auto pf, int nb) __attribute__((always_inline)) {
        constexpr bool PREFETCH = decltype(pf)::value;
        const QElem *sq = reinterpret_cast<const QElem *>(smem);
        uint32_t *bm = reinterpret_cast<uint32_t *>(smem + (size_t)sp.q_cap * sizeof(QElem)) + wave * sp.bm_words;
        const QElem *re = reinterpret_cast<const QElem *>(g.rows);
        const int mine = nb > wave ? (nb - wave + kHnswWaves - 1) / kHnswWaves : 0;  // <= 50 < 64: one lane per row
        if (mine == 0) return;
        const int ij = wave + kHnswWaves * lane;
        const int32_t ej = bi[ij < nb ? ij : nb - 1];  // never predicate a load (see scan_kernel)
        const int64_t rbj = sp.row_ptr[ej];
        const int rnj = (int)(sp.row_ptr[ej + 1] - rbj);
        RegRow cur;
        if constexpr (PREFETCH) load_reg_row(cur, re + __shfl(rbj, 0), __shfl(rnj, 0), lane);
        for (int j = 0; j < mine; j++) {
            const int64_t rb = __shfl(rbj, j);
            const int rn = __shfl(rnj, j);
            RegRow nxt;
            if constexpr (PREFETCH) {
                const int jn = j + 1 < mine ? j + 1 : j;  // (the last trip asks for its own row again)
                load_reg_row(nxt, re + __shfl(rbj, jn), __shfl(rnj, jn), lane);
            } else {
                load_reg_row(cur, re + rb, rn, lane);
            }
            float v;
            if constexpr (METRIC == 0)
                v = score_element<0>(cur, re + rb, rn, sq, sqn, bm, lane);
            else if constexpr (METRIC == 1)
                v = score_element<1>(cur, re + rb, rn, sq, sqn, bm, lane);
            else
                v = score_element<2>(cur, re + rb, rn, sq, sqn, bm, lane);
            if (lane == kWave - 1) bk[wave + kHnswWaves * j] = float_to_key(v);
            if constexpr (PREFETCH) cur = nxt;
        }
    };
    // (always inlined: as a called function -- what the fp16 instantiations got -- every batch of a walk saved and
    // restored registers through 208 bytes of scratch)
    auto score_batch = [&](int nb) __attribute__((always_inline)) {
        if constexpr (kSparse) {
            if (sp.prefetch)
                score_sparse(std::true_type{}, nb);
            else
                score_sparse(std::false_type{}, nb);
        } else {
            if (run.rows_per_trip >= 4)
                score_rows(std::integral_constant<int, 4>{}, std::false_type{}, nb);
            else if (run.rows_per_trip == 2)
                score_rows(std::integral_constant<int, 2>{}, std::false_type{}, nb);
            else
                score_rows(std::integral_constant<int, 1>{}, std::false_type{}, nb);
        }
    };

    // ---- The steps of a walk, in the order the query loop below takes them.  Always inlined, like score_batch.  The two
    // marked "wavefront 0" run under wave == 0 and hold no barrier; all 256 threads call the others.

    // the query into LDS (the caller's next barrier publishes it)
    auto stage_query = [&](int qi) __attribute__((always_inline)) {
        if constexpr (kSparse) {
            QElem *sq = reinterpret_cast<QElem *>(smem);
            if constexpr (ELEMQ) {
                // the build: the query is an element of the mirror, its pairs already side by side at g.rows
                const int32_t e = run.qids[qi];
                const int64_t qb = sp.row_ptr[e];
                sqn = (int)(sp.row_ptr[e + 1] - qb);
                const QElem *src = reinterpret_cast<const QElem *>(g.rows) + qb;
                for (int v = tid; v < sqn; v += kHnswThreads) {
                    const QPair raw = *reinterpret_cast<const QPair *>(src + v);
                    sq[v] = {raw.x, __int_as_float(raw.y)};
                }
            } else {
                const int64_t qb = sp.q_ptr[qi];
                sqn = (int)(sp.q_ptr[qi + 1] - qb);
                for (int v = tid; v < sqn; v += kHnswThreads) sq[v] = {sp.q_idx[qb + v], sp.q_val[qb + v]};
            }
        } else {
            const char *qrow = run.qids ? g.rows + (size_t)run.qids[qi] * row_bytes : run.queries + (size_t)qi * row_bytes;
            for (int v = tid; v < g.nvec; v += kHnswThreads) lq[v] = load16(qrow + (size_t)v * sizeof(Raw16));
        }
    };
    // the entry point is the first batch, and W to begin with
    auto enter_graph = [&]() __attribute__((always_inline)) {
        if (tid == 0) bi[0] = g.entry;
        __syncthreads();
        score_batch(1);
        __syncthreads();
        if (tid == 0) {
            wk[0] = bk[0];
            wi[0] = (uint32_t)g.entry;
            sc.wn = 1;
            sc.cur = 0;
        }
    };
    // a fresh visited set holding the layer's entry points (src/hnswutils.c:866-885): the previous layer's W, all
    // unexpanded again
    auto reset_visited = [&]() __attribute__((always_inline)) {
        for (int w = tid; w < words; w += kHnswThreads) bitmap[w] = 0u;
        __syncthreads();
        const int cur = sc.cur, wn = sc.wn;
        for (int j = tid; j < wn; j += kHnswThreads) {
            const uint32_t id = wi[cur * ef + j] & ~kExpanded;
            wi[cur * ef + j] = id;
            atomicOr(&bitmap[id >> 5], 1u << (id & 31));
        }
    };
    // wavefront 0: the next candidate -- W's first unexpanded entry, or with W exhausted an evicted one tied with its
    // furthest -- into sc.cand, and its unvisited neighbours at layer lc, in tuple order, into bi[0 .. sc.nb)
    auto next_candidate = [&](int lc, int lm) __attribute__((always_inline)) {
        uint32_t *ci = wi + sc.cur * ef;
        const int wn = sc.wn;
        int found = -1;
        for (int base = 0; base < wn && found < 0; base += kWave) {
            const int j = base + lane;
            const bool open = j < wn && !(ci[j] & kExpanded);
            const unsigned long long bal = __ballot(open);
            if (bal) found = base + __ffsll((long long)bal) - 1;
        }
        int nb = 0, cand = -1;
        if (found >= 0) {
            cand = (int)ci[found];
            if (lane == 0) ci[found] = (uint32_t)cand | kExpanded;
        } else if (sc.tread < sc.tn) {
            cand = (int)ti[sc.tread];
            if (lane == 0) sc.tread = sc.tread + 1;
        }
        if (cand >= 0) {
            const uint32_t c = (uint32_t)cand;
            // neighbour tuple slice of layer lc (src/hnswutils.c:786)
            const int64_t start = g.nbr_start[c] + (int64_t)(g.levels[c] - lc) * g.m;
            for (int base = 0; base < lm; base += kWave) {
                const int j = base + lane;
                const int32_t e = j < lm ? g.nbr[start + j] : -1;
                bool fresh = false;
                if (e >= 0) {
                    const uint32_t bit = 1u << (e & 31);
                    fresh = !(atomicOr(&bitmap[e >> 5], bit) & bit);
                }
                const int slot = wave_append(fresh, lane, nb);
                if (fresh) bi[slot] = e;
            }
        }
        if (lane == 0) {
            sc.nb = nb;
            sc.cand = cand;
        }
    };
    // wavefront 0: the stable merge of the scored batch into W's other buffer, truncated to ef_l; what leaves W at its
    // furthest key goes to T, and what leaves a scan's layer 0 to the query's pool.  Every slot comes from MergePos.
    auto merge_batch = [&](int qi, int lc, int ef_l, int nb) __attribute__((always_inline)) {
        const int cur = sc.cur, nxt = cur ^ 1, wn = sc.wn;
        const uint32_t *ck = wk + cur * ef, *ci = wi + cur * ef;
        uint32_t *nk = wk + nxt * ef, *ni = wi + nxt * ef;
        // "make robust to issues" (src/hnswutils.c:947-949): an element below this layer is scored and stays visited
        // but is never admitted; only upper layers can see one.  They leave the batch here, the order kept.
        if (lc > 0) {
            int kept = 0;
            for (int base = 0; base < nb; base += kWave) {
                const int i = base + lane;
                const bool keep = i < nb && g.levels[bi[i < nb ? i : 0]] >= lc;
                const uint32_t key = i < nb ? bk[i] : 0u;
                const int32_t id = i < nb ? bi[i] : 0;
                const int slot = wave_append(keep, lane, kept);
                // in-place compaction is safe: a chunk only writes at or below its own reads
                if (keep) {
                    bk[slot] = key;
                    bi[slot] = id;
                }
            }
            nb = kept;
        }
        const MergePos pos{ck, bk, wn, nb};
        const int wn_new = wn + nb < ef_l ? wn + nb : ef_l;
        auto to_w = [&](int s, uint32_t key, uint32_t id) __attribute__((always_inline)) {
            if (s < ef_l) {
                nk[s] = key;
                ni[s] = id;
            }
        };
        for (int j = lane; j < wn; j += kWave) to_w(pos.old_slot(j, ck[j]), ck[j], ci[j]);
        for (int i = lane; i < nb; i += kWave) to_w(pos.batch_slot(i, bk[i]), bk[i], (uint32_t)bi[i]);
        // The tie list.  With W full, its furthest key K is nk[ef_l - 1].  T keeps the unexpanded candidates that were
        // pushed out of W at exactly K: old entries, and batch entries that had been admitted when their turn came (fewer
        // than ef_l entries not farther among W and the batch entries before them).  Entries of an older T stay only if K
        // has not moved.
        if (wn_new == ef_l && wn + nb > ef_l) {
            const uint32_t K = nk[ef_l - 1];
            int tn = sc.tn;
            if (tn > 0 && sc.tkey != K) tn = 0;
            const int t0 = tn > 0 ? sc.tread : 0;
            auto to_t = [&](bool tie, uint32_t id) __attribute__((always_inline)) {
                const int slot = wave_append(tie, lane, tn);
                if (tie && slot < ef) ti[slot] = id;  // (slot < ef always: the guard only keeps a write inside T)
            };
            for (int base = 0; base < wn; base += kWave) {
                const int j = base + lane;
                const bool live = j < wn && ck[j] == K && !(ci[j] & kExpanded);
                to_t(live && pos.old_slot(j, K) >= ef_l, live ? ci[j] : 0u);
            }
            for (int base = 0; base < nb; base += kWave) {
                const int i = base + lane;
                const bool at_k = i < nb && bk[i] == K;
                int before = 0;  // admitted in its turn, pushed out later:
                to_t(at_k && pos.batch_slot(i, K, before) >= ef_l && before < ef_l, at_k ? (uint32_t)bi[i] : 0u);
            }
            if (lane == 0) {
                sc.tn = tn < ef ? tn : ef;  // (tn < ef always: nothing is truncated)
                sc.tread = t0;
                sc.tkey = K;
            }
        }
        // A scan keeps what the merge leaves past position ef (`discarded`, src/hnswutils.c:936-946, :967-973; layer 0
        // only, src/hnswscan.c:55): the old entries pushed out, in W's order, then the batch entries that did not fit,
        // in batch order -- whether or not they also went to T.  Never written past the pool: the count goes on, and
        // the batch ends flagged.
        if constexpr (SCAN) {
            if (lc == 0 && wn + nb > ef_l) {
                uint2 *pool = ss.pool + (size_t)qi * ss.cap;
                int pn = sc.pool_n;
                auto to_pool = [&](bool out, uint2 e) __attribute__((always_inline)) {
                    const int slot = wave_append(out, lane, pn);
                    if (out && slot < ss.cap) pool[slot] = e;
                };
                // (an old entry moves up by at most nb: only W's last nb entries can leave)
                for (int base = ef_l > nb ? ef_l - nb : 0; base < wn; base += kWave) {
                    const int j = base + lane;
                    const uint2 e = {j < wn ? ck[j] : 0u, j < wn ? ci[j] & ~kExpanded : 0u};
                    to_pool(j < wn && pos.old_slot(j, e.x) >= ef_l, e);
                }
                for (int base = 0; base < nb; base += kWave) {
                    const int i = base + lane;
                    const uint2 e = {i < nb ? bk[i] : 0u, i < nb ? (uint32_t)bi[i] : 0u};
                    to_pool(i < nb && pos.batch_slot(i, e.x) >= ef_l, e);
                }
                if (lane == 0) sc.pool_n = pn;
            }
        }
        if (lane == 0) {
            sc.wn = wn_new;
            sc.cur = nxt;
        }
    };
    // a build's query: layer lc's W, the candidates SelectNeighbors sees
    auto hand_out_w = [&](int qi, int lc) __attribute__((always_inline)) {
        const int cur = sc.cur, wn = sc.wn;
        const size_t o = ((size_t)qi * run.lcap + lc) * ef;
        for (int j = tid; j < wn; j += kHnswThreads) {
            run.lw_ids[o + j] = (int32_t)(wi[cur * ef + j] & ~kExpanded);
            if constexpr (!kJaccard) run.lw_dist[o + j] = key_to_float(wk[cur * ef + j]);
        }
        // a Jaccard build: W is ordered by the key (the float8's order, what HnswSearchLayer leaves), the list's
        // distances are the (float) of the float8 (HnswCandidate.distance, src/hnswutils.c:1336), which the key does
        // not carry -- W meets the query once more.  Distinct keys may give equal floats; the order stays.
        jaccard_out(wi + cur * ef, wn, run.lw_dist + o);
        if (tid == 0) run.lw_cnt[(size_t)qi * run.lcap + lc] = wn;
    };
    // The epilogue: query qi's results are ids[0 .. cnt) (expanded flags off), nearest first (src/hnswscan.c:293-311),
    // and the distances their keys stand for; -1 / +inf from cnt on.  A Jaccard walk scores them once more against the
    // query, which is in LDS.  cnt == 0: ids and keys are not read.
    auto write_results = [&](int qi, const uint32_t *ids, const uint32_t *keys, int cnt) __attribute__((always_inline)) {
        if (!out_elem) return;
        if (cnt > k) cnt = k;
        // (a signed row offset: with (size_t)qi * k + j in this lambda every instantiation took six more VGPRs than with
        // the same statements written out at each site, and seven of them lost a wavefront per SIMD)
        const int64_t row = (int64_t)qi * k;
        for (int j = tid; j < k; j += kHnswThreads) {
            const bool have = j < cnt;
            out_elem[row + j] = have ? (int64_t)(ids[j] & ~kExpanded) : -1;
            if (!have)
                out_dist[row + j] = __uint_as_float(0x7f800000u);
            else if constexpr (!kJaccard)
                out_dist[row + j] = key_to_float(keys[j]);
        }
        jaccard_out(ids, cnt, out_dist + row);
    };
    // A filtered scan's walk of the staged query (FILTER): into the graph and down its layers, or -- a resumed batch, W
    // laid out by the entry step -- layer 0 alone.  Leaves W in buffer sc.cur, sc.wn entries; counts so->tuples into
    // `scored`.  The query loop's own layer loop below, less what only a build asks for; that one stays written out where
    // it is: with both paths calling one lambda every older instantiation spilled a different number of SGPRs and two of
    // them changed their VGPR count.
    auto walk_layers = [&](int qi, bool resumed, int64_t &scored) __attribute__((always_inline)) {
        if constexpr (FILTER) {
            if (!resumed) enter_graph();
            for (int lc = resumed ? 0 : g.levels[g.entry]; lc >= 0; lc--) {
                const int ef_l = lc == 0 ? ef : 1;
                const int lm = lc == 0 ? lm0 : g.m;
                if (!resumed) reset_visited();  // (a resumed batch keeps its visited set: initVisited == false)
                if (tid == 0) sc.tn = sc.tread = 0;
                __syncthreads();
                if (lc == 0 && !resumed) scored += sc.wn;  // its entry points count too (src/hnswutils.c:872-873)
                for (;;) {
                    if (wave == 0) next_candidate(lc, lm);
                    __syncthreads();
                    const int nb = sc.nb;
                    if (sc.cand < 0) break;
                    if (nb == 0) {
                        __syncthreads();
                        continue;
                    }
                    if (lc == 0) scored += nb;
                    score_batch(nb);
                    __syncthreads();
                    if (wave == 0) merge_batch(qi, lc, ef_l, nb);
                    __syncthreads();
                }
                __syncthreads();
            }
        }
    };
    // A filtered scan's step after each walk or drain (FILTER; hnswgettuple's inner loop, src/hnswscan.c:293-327): W's
    // live buffer nearest first through strict_order and the query's keep bitmap, the survivors into the output row at
    // `emitted`, k rows at the most -- the rest of the batch is dropped.  Wavefront 0 compacts them into W's other buffer,
    // which is dead between two batches; all 256 threads write them out.  A batch is ascending, so an entry passes
    // strict_order exactly when it is not nearer than the last key that passed before the batch, and the batch's last key
    // is the next such key unless nothing passed.  All 256 threads call, after a barrier; ends with one.
    // `emitted` is the same register in every thread: wavefront 0 publishes only the batch's count, sc.got, which nobody
    // reads before the barrier behind it and nobody writes again before the next batch's, and every thread adds it.
    auto filter_batch = [&](int qi, const uint32_t *keep, int &emitted) __attribute__((always_inline)) {
        if constexpr (FILTER) {
            const int cur = sc.cur, wn = sc.wn, e0 = emitted;
            uint32_t *dk = wk + (cur ^ 1) * ef, *di = wi + (cur ^ 1) * ef;
            if (wave == 0) {
                const uint32_t *ck = wk + cur * ef, *ci = wi + cur * ef;
                const uint32_t prev = sc.prev;
                const int room = k - e0;
                int cnt = 0;
                for (int base = 0; base < wn && cnt < room; base += kWave) {
                    const int j = base + lane < wn ? base + lane : wn - 1;  // never predicate a load
                    const uint32_t key = ck[j], id = ci[j] & ~kExpanded;
                    bool ok = base + lane < wn && (!ss.strict || key >= prev);
                    if (keep) ok = ok && ((keep[id >> 5] >> (id & 31)) & 1u);
                    const int slot = wave_append(ok, lane, cnt);
                    if (ok && slot < room) {
                        dk[slot] = key;
                        di[slot] = id;
                    }
                }
                if (lane == 0) {
                    sc.got = cnt < room ? cnt : room;
                    if (ss.strict && wn > 0 && ck[wn - 1] > prev) sc.prev = ck[wn - 1];
                    sc.batches = sc.batches + 1;
                }
            }
            __syncthreads();
            const int got = sc.got;
            const int64_t at = (int64_t)qi * k + e0;
            for (int j = tid; j < got; j += kHnswThreads) {
                out_elem[at + j] = (int64_t)di[j];
                if constexpr (!kJaccard) out_dist[at + j] = key_to_float(dk[j]);
            }
            jaccard_out(di, got, out_dist + at);  // (the kept elements meet the query once more: it is in LDS)
            emitted = e0 + got;
            __syncthreads();
        }
    };

    for (;;) {
        if (tid == 0) sc.query = atomicAdd(qcounter, 1);
        __syncthreads();
        const int qi = sc.query;
        if (qi >= nq) return;

        int64_t scored = 0;
        // A filtered scan's query (FILTER) is hnswgettuple's loop, start to end: a batch -- the first walk, a resumed one,
        // or with so->tuples at max_scan_tuples the entry step alone -- then the filter, until k rows are out, the pool
        // is empty or it has overflowed.  The query is staged once; its state is written once, when it stops, with the
        // fields a batch of pgv_hnsw_scan_next writes.  Every batch but the first takes at least one entry out of the
        // pool and the walks mark new elements visited: a query ends after n elements' worth of work at the most.
        if constexpr (FILTER) {
            bitmap = bitmaps + (size_t)qi * words;
            const HnswScanQuery st = ss.qs[qi];
            const bool wanted = (!ss.want || ss.want[qi]) && !(st.flags & kScanOverflow) && g.entry >= 0;
            bool started = st.flags & kScanStarted, over = false;
            int emitted = 0;
            scored = st.tuples;
            if (tid == 0) {
                sc.pool_n = st.pool_n;
                sc.prev = 0u;
                sc.batches = 0;
            }
            if (wanted) stage_query(qi);
            __syncthreads();
            if (wanted) {
                const uint32_t *keep = ss.keep ? ss.keep + (int64_t)qi * ss.keep_stride : nullptr;
                uint2 *pool = ss.pool + (size_t)qi * ss.cap;
                for (;;) {
                    const int pn = sc.pool_n;
                    if (emitted >= k || (started && pn == 0)) break;
                    const bool drain = started && scored >= ss.max_tuples;
                    if (started) {
                        const int take = pn < ef ? pn : ef;
                        scan_entry_step(pool, pn, take, wk, wi, wk + ef, wi + ef, *reinterpret_cast<ScanEntryLds *>(smem + at.entry));
                        if (tid == 0) {
                            sc.wn = take;
                            sc.cur = 0;
                            sc.pool_n = pn - take;
                        }
                        __syncthreads();
                    }
                    if (!drain) walk_layers(qi, started, scored);
                    started = true;
                    filter_batch(qi, keep, emitted);
                    if (sc.pool_n > ss.cap) {  // the pool overflowed in this walk: the query ends flagged
                        over = true;
                        break;
                    }
                }
            }
            const int em = emitted;
            const int64_t row = (int64_t)qi * k;
            for (int j = em + tid; j < k; j += kHnswThreads) {
                out_elem[row + j] = -1;
                out_dist[row + j] = __uint_as_float(0x7f800000u);
            }
            if (tid == 0) {
                const int pn = over ? ss.cap : sc.pool_n;
                ss.out_count[qi] = em;
                if (out_scored) out_scored[qi] = scored;
                if (ss.out_batches) ss.out_batches[qi] = sc.batches;
                if (ss.out_left) ss.out_left[qi] = pn;
                if (sc.batches > 0) ss.qs[qi] = {scored, pn, kScanStarted | (over ? kScanOverflow : 0)};
                if (over) atomicCAS(ss.overflow, 0, qi + 1);
            }
            __syncthreads();
            continue;
        }
        // A scan's query (SCAN): not wanted, exhausted, over an empty index or flagged -> no batch, its state stays as it
        // is.  A started one resumes: the entry step lays the pool's nearest into W, the visited set carries over, the
        // upper layers are not walked again (ResumeScanItems, src/hnswscan.c:61-87).  A drain is the entry step alone.
        bool resumed = false;
        if constexpr (SCAN) {
            bitmap = bitmaps + (size_t)qi * words;
            const HnswScanQuery st = ss.qs[qi];
            const bool started = st.flags & kScanStarted;
            const bool wanted = (!ss.want || ss.want[qi]) && !(st.flags & kScanOverflow) && g.entry >= 0;
            const bool live = wanted && (ss.drain ? st.pool_n > 0 : (!started || st.pool_n > 0));
            if (!live) {
                write_results(qi, nullptr, nullptr, 0);
                if (tid == 0) {
                    ss.out_count[qi] = 0;
                    if (out_scored) out_scored[qi] = st.tuples;
                    if (ss.out_left) ss.out_left[qi] = st.pool_n;
                }
                __syncthreads();
                continue;
            }
            resumed = started;
            scored = st.tuples;
            if (tid == 0) sc.pool_n = st.pool_n;
            if (resumed) {
                const int take = st.pool_n < ef ? st.pool_n : ef;
                scan_entry_step(ss.pool + (size_t)qi * ss.cap, st.pool_n, take, wk, wi, wk + ef, wi + ef,
                                *reinterpret_cast<ScanEntryLds *>(smem + at.entry));
                if (tid == 0) {
                    sc.wn = take;
                    sc.cur = 0;
                    sc.pool_n = st.pool_n - take;
                }
                __syncthreads();
                if (ss.drain) {
                    if constexpr (kJaccard) {  // (the pool keeps keys: the drained elements meet the query once more)
                        stage_query(qi);
                        __syncthreads();
                    }
                    write_results(qi, wi, wk, take);
                    if (tid == 0) {
                        ss.out_count[qi] = take;
                        if (ss.out_left) ss.out_left[qi] = st.pool_n - take;
                        ss.qs[qi].pool_n = st.pool_n - take;
                    }
                    __syncthreads();
                    continue;
                }
            }
        }
        const int qlevel = run.qlevels ? run.qlevels[qi] : 0;
        if (run.lw_cnt)
            for (int l = tid; l < run.lcap; l += kHnswThreads) run.lw_cnt[(size_t)qi * run.lcap + l] = 0;
        if (g.entry < 0) {  // empty index
            write_results(qi, nullptr, nullptr, 0);
            if (tid == 0 && out_scored) out_scored[qi] = 0;
            __syncthreads();
            continue;
        }

        stage_query(qi);
        if (!SCAN || !resumed) enter_graph();
        const int top = SCAN && resumed ? 0 : g.levels[g.entry];

        for (int lc = top; lc >= 0; lc--) {
            const int ef_l = lc <= qlevel ? ef : 1;
            const int lm = lc == 0 ? lm0 : g.m;
            // (a resumed batch of a scan keeps its visited set; its entry points are in it and were counted when they
            // were scored: initVisited == false, src/hnswutils.c:867-874)
            if (!SCAN || !resumed) reset_visited();
            if (tid == 0) sc.tn = sc.tread = 0;
            __syncthreads();
            if (lc == 0 && (!SCAN || !resumed)) scored += sc.wn;  // its entry points count too (src/hnswutils.c:872-873)

            for (;;) {
                if (wave == 0) next_candidate(lc, lm);
                __syncthreads();
                const int nb = sc.nb;
                if (sc.cand < 0) break;  // every entry of W expanded: the reference's C is exhausted or too far
                if (nb == 0) {
                    __syncthreads();
                    continue;
                }
                if (lc == 0) scored += nb;  // so->tuples: only the layer-0 search counts (src/hnswscan.c:52-55)
                score_batch(nb);
                __syncthreads();
                if (wave == 0) merge_batch(qi, lc, ef_l, nb);
                __syncthreads();
            }
            __syncthreads();
            if (run.lw_ids && lc <= qlevel && lc < run.lcap) hand_out_w(qi, lc);
        }

        write_results(qi, wi + sc.cur * ef, wk + sc.cur * ef, sc.wn);
        if (tid == 0 && out_scored) out_scored[qi] = scored;
        if constexpr (SCAN) {
            if (tid == 0) {
                const int pn = sc.pool_n;
                const bool over = pn > ss.cap;
                ss.out_count[qi] = sc.wn;
                if (ss.out_left) ss.out_left[qi] = over ? ss.cap : pn;
                ss.qs[qi] = {scored, over ? ss.cap : pn, kScanStarted | (over ? kScanOverflow : 0)};
                if (over) atomicCAS(ss.overflow, 0, qi + 1);
            }
        }
        __syncthreads();
    }
}

// neighbour tuples of a few elements rewritten in place (the build's graph grows batch by batch);
// a tuple the caller sized wrongly or an element out of range is skipped
__global__ __launch_bounds__(256) void hnsw_patch_kernel(int32_t *__restrict__ nbr, const int64_t *__restrict__ nbr_start,
                                                          int64_t n, const int32_t *__restrict__ ids,
                                                          const int64_t *__restrict__ packed_off,
                                                          const int32_t *__restrict__ packed, int nupd) {
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= nupd) return;
    const int32_t e = ids[wave];
    if (e < 0 || e >= n) return;
    const int64_t dst = nbr_start[e], len = nbr_start[e + 1] - dst, src = packed_off[wave];
    if (packed_off[wave + 1] - src != len) return;
    for (int64_t j = lane; j < len; j += 64) nbr[dst + j] = packed[src + j];
}

// the LDS a walk over sparse rows needs (*lds_out, may be NULL), against the limit: the text names ef, m and the query length
int hnsw_sparse_lds_check(const char *who, int ef, int m, int q_cap, int bm_words, bool scan, size_t *lds_out) {
    const size_t lds = HnswLds(sparse_query_bytes(q_cap, bm_words), ef, m, scan).total;
    if (lds_out) *lds_out = lds;
    if (lds > kHnswLdsLimit)
        PGV_FAIL(PGV_ERR_ARG, "%s: ef %d / m %d / a query of %d stored elements need %zu bytes of LDS (limit %d)", who, ef, m,
                 q_cap, lds, (int)kHnswLdsLimit);
    return PGV_OK;
}

template <typename T, int METRIC, typename Last = HnswSparse, bool ELEMQ = false>
int launch_hnsw_t(pgv_ctx *ctx, const HnswDev &g, const HnswRun &run, uint32_t *bitmaps, int words, int grid,
                  int *counter, const Last &sp = Last{}) {
    constexpr bool kSparse = std::is_same_v<T, SparseRow>;
    constexpr bool kScan = std::is_base_of_v<HnswScanDev, Last>;
    constexpr bool kFilter = kIsFiltered<Last>;
    static_assert(std::is_same_v<Last, HnswLast<T, kScan, kFilter>>, "the kernel's last argument for these rows");
    size_t lds = HnswLds((size_t)g.nvec * sizeof(Raw16), run.ef, g.m, kScan).total;  // the layout the kernel carves
    if constexpr (kSparse) {
        const HnswSparse none{};
        const HnswSparse &extras = sparse_extras(sp, none);
        PGV_TRY(hnsw_sparse_lds_check(kScan ? "hnsw scan" : "hnsw search", run.ef, g.m, extras.q_cap, extras.bm_words, kScan, &lds));
    } else if (lds > kHnswLdsLimit) {
        PGV_FAIL(PGV_ERR_ARG, "hnsw search: ef %d / m %d need %zu bytes of LDS", run.ef, g.m, lds);
    }
    auto kern = hnsw_search_kernel<T, METRIC, kScan, ELEMQ, kFilter>;
    PGV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kHnswThreads), lds, ctx->stream, g, run, bitmaps, words, counter, sp);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}


// ------------------------------------------------------------------ SelectNeighbors for the elements being inserted
// HnswFindElementNeighbors ends each layer with SelectNeighbors(w, lm, ...) (src/hnswutils.c:1064-1165, Algorithm 4 of
// the HNSW paper with the reference's extras) over the layer's candidate list W, and CheckElementCloser (:1040-1059)
// inside it compares the candidate's distance to the element with its distances to the neighbors chosen so far.  For a
// NEW element the list has no cached `closer` flags (closerSet is false: every check is computed) and W arrives ordered
// by the search, so the selection is the plain greedy sweep, nearest candidate first:
//     closer(e) = no neighbor r chosen so far has d(e, r) <= d(e, q)          (ties are NOT closer: `<=` at :1053)
//     chosen while |r| < lm; the rejected ones ("pruned connections", :1146-1148) fill r up to lm, nearest first
// and a list of at most lm candidates is taken whole, in W's own (furthest first) order (:1072-1073).
//
// Three launches on the searches' stream: which lists need thinning and where their pair triangles go (one workgroup:
// an exclusive scan), those lists' (u, v < u) distances (score_groups_kernel, or expand_groups_kernel's slot pairs
// through score_gather_kernel), and the sweep itself, one lane per list: its inner loop is a dependent chain of
// comparisons, the lists of a batch are thousands, and a wavefront's 64 lists share nothing, so lanes are the
// parallelism.

// pairs of list g = (query, layer): cnt * (cnt - 1) / 2 when it has to be thinned, else none; start[] by exclusive scan
// (256 threads: a larger workgroup waits for a whole CU's worth of room while another stream's searches fill the chip)
__global__ __launch_bounds__(256) void hnsw_select_plan_kernel(const int32_t *__restrict__ cnt, int ngroups, int lcap, int m,
                                                                int64_t *__restrict__ pair_start) {
    constexpr int T = 256, PER = 8;
    __shared__ int64_t wave_tot[T / 64];
    __shared__ int64_t carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < ngroups; base += T * PER) {
        const int g0 = base + (int)threadIdx.x * PER;
        int64_t v[PER], mine = 0;
#pragma unroll
        for (int t = 0; t < PER; t++) {
            const int g = g0 + t;
            v[t] = 0;
            if (g < ngroups) {
                const int lm = (g % lcap) == 0 ? 2 * m : m;
                const int64_t c = cnt[g];
                v[t] = c > lm ? c * (c - 1) / 2 : 0;
            }
            mine += v[t];
        }
        int64_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int64_t before = 0, total = 0;
        for (int w = 0; w < T / 64; w++) {
            const int64_t t = wave_tot[w];
            if (w < wave) before += t;
            total += t;
        }
        const int64_t carry = carry_s;
        int64_t run = carry + before + incl - mine;
#pragma unroll
        for (int t = 0; t < PER; t++) {
            if (g0 + t < ngroups) pair_start[g0 + t] = run;
            run += v[t];
        }
        __syncthreads();
        if (threadIdx.x == 0) carry_s = carry + total;
        __syncthreads();
    }
    if (threadIdx.x == 0) pair_start[ngroups] = carry_s;
}

// the sweep: list g's candidates are lw_ids / lw_dist[g * ef ..), nearest first; tri = its pair distances.
// out_* [g * stride ..): the neighbors in the order the reference's r holds them, their distances, their closer flags
__global__ __launch_bounds__(64) void hnsw_select_kernel(const int32_t *__restrict__ lw_ids, const float *__restrict__ lw_dist,
                                                         const int32_t *__restrict__ cnt, const int32_t *__restrict__ qlevels,
                                                         const int64_t *__restrict__ pair_start, const float *__restrict__ tri_all,
                                                         int ngroups, int lcap, int ef, int m, int stride,
                                                         int32_t *__restrict__ out_ids, float *__restrict__ out_dist,
                                                         uint8_t *__restrict__ out_closer, int32_t *__restrict__ out_cnt) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= ngroups) return;
    const int lc = g % lcap, q = g / lcap;
    const int lm = lc == 0 ? 2 * m : m;
    const int nw = lc > qlevels[q] ? 0 : cnt[g];  // (layers above the insert level are descended, not linked)
    const int32_t *ids = lw_ids + (size_t)g * ef;
    const float *dist = lw_dist + (size_t)g * ef;
    int32_t *oi = out_ids + (size_t)g * stride;
    float *od = out_dist + (size_t)g * stride;
    uint8_t *oc = out_closer + (size_t)g * stride;
    if (nw <= lm) {
        // taken whole, in W's order: furthest first
        for (int i = 0; i < nw; i++) {
            oi[i] = ids[nw - 1 - i];
            od[i] = dist[nw - 1 - i];
            oc[i] = 0;
        }
        out_cnt[g] = nw;
        return;
    }
    const float *tri = tri_all + pair_start[g];
    int rn = 0;
    // the chosen ones' candidate indexes live in the output (their ids are written there anyway): oi[i] holds the
    // INDEX until the end, then the element
    int j = 0;
    for (; j < nw && rn < lm; j++) {
        const float de = dist[j];
        bool closer = true;
        for (int i = 0; i < rn; i++) {
            const int r = oi[i];  // r < j: chosen earlier, nearer or equal
            if (tri[(int64_t)j * (j - 1) / 2 + r] <= de) {
                closer = false;
                break;
            }
        }
        if (closer) oi[rn++] = j;
    }
    // the candidates looked at are 0 .. j - 1; the rejected among them, nearest first, fill r up to lm.  Walk them by
    // merging "all of 0 .. j - 1" against the chosen (ascending) indexes.
    const int chosen = rn;
    {
        int ci = 0;
        for (int x = 0; x < j && rn < lm; x++) {
            if (ci < chosen && oi[ci] == x) {
                ci++;
                continue;
            }
            oi[rn++] = x;
        }
    }
    for (int i = 0; i < rn; i++) {
        const int x = oi[i];
        od[i] = dist[x];
        oc[i] = i < chosen ? 1 : 0;
        oi[i] = ids[x];
    }
    out_cnt[g] = rn;
}


// the same sweep, one WAVEFRONT per list, for ef_construction <= 64: lane j holds candidate j, the list's pair triangle sits
// in LDS, and "no neighbor chosen so far is at distance <= mine" is one comparison per chosen lane and a ballot.  What
// stays sequential is the walk over the candidates, nearest first.
__global__ __launch_bounds__(256) void hnsw_select_wave_kernel(const int32_t *__restrict__ lw_ids, const float *__restrict__ lw_dist,
                                                               const int32_t *__restrict__ cnt, const int32_t *__restrict__ qlevels,
                                                               const int64_t *__restrict__ pair_start,
                                                               const float *__restrict__ tri_all, int ngroups, int lcap, int ef,
                                                               int m, int stride, int32_t *__restrict__ out_ids,
                                                               float *__restrict__ out_dist, uint8_t *__restrict__ out_closer,
                                                               int32_t *__restrict__ out_cnt) {
    __shared__ float tri_lds[4][64 * 63 / 2 + 64];  // (+ 64: the lanes that are not chosen index past their row harmlessly)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = blockIdx.x * 4 + wv;
    if (g >= ngroups) return;
    const int lc = g % lcap, q = g / lcap;
    const int lm = lc == 0 ? 2 * m : m;
    const int nw = lc > qlevels[q] ? 0 : cnt[g];
    int32_t *oi = out_ids + (size_t)g * stride;
    float *od = out_dist + (size_t)g * stride;
    uint8_t *oc = out_closer + (size_t)g * stride;
    const int32_t id = lane < nw ? lw_ids[(size_t)g * ef + lane] : -1;
    const float dist = lane < nw ? lw_dist[(size_t)g * ef + lane] : 0.f;
    if (nw <= lm) {
        // taken whole, in W's order: furthest first
        if (lane < nw) {
            oi[nw - 1 - lane] = id;
            od[nw - 1 - lane] = dist;
            oc[nw - 1 - lane] = 0;
        }
        if (lane == 0) out_cnt[g] = nw;
        return;
    }
    const float *tri_g = tri_all + pair_start[g];
    const int np = nw * (nw - 1) / 2;
    for (int i = lane; i < np; i += 64) tri_lds[wv][i] = tri_g[i];
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    bool chosen = false;
    int pos = -1, rn = 0, nrej = 0, rpos = -1;
    for (int j = 0; j < nw && rn < lm; j++) {
        const float dj = __shfl(dist, j);
        const bool decides = chosen && tri_lds[wv][j * (j - 1) / 2 + lane] <= dj;  // (chosen lanes are < j)
        if (__ballot(decides)) {
            if (lane == j) rpos = nrej;
            nrej++;
        } else {
            if (lane == j) {
                chosen = true;
                pos = rn;
            }
            rn++;
        }
    }
    // the rejected among the candidates looked at fill r up to lm, nearest first (:1146-1148)
    const int nchosen = rn;
    if (rpos >= 0 && nchosen + rpos < lm) pos = nchosen + rpos;
    const int total = nchosen + nrej < lm ? nchosen + nrej : lm;
    if (pos >= 0) {
        oi[pos] = id;
        od[pos] = dist;
        oc[pos] = chosen ? 1 : 0;
    }
    if (lane == 0) out_cnt[g] = total;
}

}  // namespace

// Lanes per bit row.  row_geom minimises wasted lane-trips of rows that are hundreds of vectors long; a bit row is 1 to
// 500 vectors (1536 bits: 12), a walk's batch is at most 2 m of them, and a batch costs what its longest chain of
// dependent loads costs.  So a row is spread over the smallest power of two of lanes that covers it in ONE trip (every
// vector of every row of a batch in flight at once; the idle lanes of a 12-vector row on 16 lanes cost nothing a
// latency-bound walk would notice), a whole wavefront in ceil(nvec / 64) <= 8 trips past 64 vectors (8192 bits).
RowGeom bit_row_geom(int nbits) {
    RowGeom g;
    const int bytes = (nbits + 7) / 8;
    g.nvec = (bytes + kVecBytes - 1) / kVecBytes;
    if (g.nvec < 1) g.nvec = 1;
    g.ld = g.nvec * kVecBytes;
    g.lpr_log2 = 0;
    while (g.lpr_log2 < 6 && (1 << g.lpr_log2) < g.nvec) g.lpr_log2++;
    g.nchunks = (g.nvec + (1 << g.lpr_log2) - 1) >> g.lpr_log2;
    return g;
}

int hnsw_search_grid(pgv_ctx *ctx, int nq, int64_t n, int *words_out) {
    const int words = (int)((n + 31) / 32) + 1;
    int grid = ctx->num_cus * 4;
    const int64_t cap = (int64_t)(1ll << 30) / ((int64_t)words * 4);  // visited bitmaps: <= 1 GiB
    if (grid > cap) grid = cap > 0 ? (int)cap : 1;
    if (grid > nq) grid = nq;
    *words_out = words;
    return grid;
}

int launch_hnsw_search(pgv_ctx *ctx, const RowsView &v, const HnswGraph &graph, const HnswSearchArgs &a, uint32_t *bitmaps,
                       int words, int grid, int *counter, const HnswScanArgs *scan) {
    // the rows, the graph and one launch's queries and outputs as the kernel takes them
    HnswDev g;
    g.rows = static_cast<const char *>(v.rows);
    g.nvec = v.geom.nvec;
    g.lpr_log2 = v.geom.lpr_log2;
    g.nchunks = v.geom.nchunks;
    g.levels = graph.levels;
    g.nbr_start = graph.nbr_start;
    g.nbr = graph.nbr;
    g.m = graph.m;
    g.entry = graph.entry;
    g.n = v.n;
    HnswRun run;
    run.queries = static_cast<const char *>(a.queries);
    run.qids = a.qids;
    run.qlevels = a.qlevels;
    run.nq = a.nq;
    run.ef = a.ef;
    run.k = a.k;
    run.out_elem = a.out_elem;
    run.out_dist = a.out_dist;
    run.out_scored = a.out_scored;
    run.lw_ids = a.lw_ids;
    run.lw_dist = a.lw_dist;
    run.lw_cnt = a.lw_cnt;
    run.lcap = a.lcap;
    static const int per_trip = getenv("PGV_HNSW_ROWS_PER_TRIP") ? atoi(getenv("PGV_HNSW_ROWS_PER_TRIP")) : 4;
    run.rows_per_trip = per_trip >= 4 ? 4 : (per_trip == 1 ? 1 : 2);
    static const int prefetch = getenv("PGV_HNSW_SPARSE_PREFETCH") ? atoi(getenv("PGV_HNSW_SPARSE_PREFETCH")) : 1;
    PGV_HIP(hipMemsetAsync(counter, 0, sizeof(int), ctx->stream));
    // what a walk over sparse rows takes on top; q_cap / bm_words from max_q_nnz: a scan's longest query, whatever it wants
    HnswSparse sp{};
    if (v.sparse()) {
        sp.row_ptr = v.ptr;
        sp.q_ptr = a.sparse_queries.ptr;
        sp.q_idx = a.sparse_queries.idx;
        sp.q_val = a.sparse_queries.val;
        sp.q_cap = pad4(a.max_q_nnz);
        sp.bm_words = v.metric == PGV_NEG_IP ? 0 : bitmap_words(a.max_q_nnz);
        sp.prefetch = prefetch != 0;
    }
    if (scan) {  // a batch of a resumable scan, or its drain: the walk's SCAN form over the scan's own state
        if (a.qids || !a.out_elem || !a.out_dist || (a.k != a.ef && !scan->filtered) || (v.sparse() && !a.sparse_queries.ptr))
            PGV_FAIL(PGV_ERR_ARG, "hnsw scan: query vectors (sparse rows: sparse queries), not element slots; k = ef");
        if (v.sparse() && a.max_q_nnz > kSparseMaxNnz)
            PGV_FAIL(PGV_ERR_DIMS, "hnsw scan: a query of %d stored elements", a.max_q_nnz);
        HnswSparseScan sd;
        sd.sp = sp;
        sd.pool = static_cast<uint2 *>(scan->pool);
        sd.cap = scan->cap;
        sd.qs = static_cast<HnswScanQuery *>(scan->qstate);
        sd.want = scan->want;
        sd.out_count = scan->out_count;
        sd.out_left = scan->out_left;
        sd.overflow = scan->overflow;
        sd.drain = scan->drain ? 1 : 0;
        if (scan->filtered) {  // hnswgettuple's whole loop per query: the FILTER forms, the scan's state wrapped
            if (scan->drain || a.k < 1) PGV_FAIL(PGV_ERR_ARG, "hnsw filtered scan: k >= 1, and it drains by itself");
            auto wrap = [&](auto base) {
                HnswFiltered<decltype(base)> f;
                static_cast<decltype(base) &>(f) = base;
                f.keep = scan->keep;
                f.keep_stride = scan->keep_stride;
                f.max_tuples = scan->max_scan_tuples;
                f.strict = scan->strict ? 1 : 0;
                f.out_batches = scan->out_batches;
                return f;
            };
            if (v.sparse()) {
                const auto f = wrap(sd);
                using F = HnswFiltered<HnswSparseScan>;
                switch (v.metric) {
                    case PGV_L2SQ: return launch_hnsw_t<SparseRow, 0, F>(ctx, g, run, bitmaps, words, grid, counter, f);
                    case PGV_NEG_IP: return launch_hnsw_t<SparseRow, 1, F>(ctx, g, run, bitmaps, words, grid, counter, f);
                    case PGV_L1: return launch_hnsw_t<SparseRow, 2, F>(ctx, g, run, bitmaps, words, grid, counter, f);
                    default: PGV_FAIL(PGV_ERR_ARG, "unknown metric %d", (int)v.metric);
                }
            }
            const auto f = wrap(static_cast<const HnswScanDev &>(sd));
            return dispatch_rows(v, [&](auto *tp, auto mc) {
                return launch_hnsw_t<std::remove_pointer_t<decltype(tp)>, decltype(mc)::value, HnswFiltered<HnswScanDev>>(
                    ctx, g, run, bitmaps, words, grid, counter, f);
            });
        }
        if (v.sparse()) switch (v.metric) {
                case PGV_L2SQ: return launch_hnsw_t<SparseRow, 0, HnswSparseScan>(ctx, g, run, bitmaps, words, grid, counter, sd);
                case PGV_NEG_IP: return launch_hnsw_t<SparseRow, 1, HnswSparseScan>(ctx, g, run, bitmaps, words, grid, counter, sd);
                case PGV_L1: return launch_hnsw_t<SparseRow, 2, HnswSparseScan>(ctx, g, run, bitmaps, words, grid, counter, sd);
                default: PGV_FAIL(PGV_ERR_ARG, "unknown metric %d", (int)v.metric);
            }
        const HnswScanDev &dense = sd;
        return dispatch_rows(v, [&](auto *tp, auto mc) {
            return launch_hnsw_t<std::remove_pointer_t<decltype(tp)>, decltype(mc)::value, HnswScanDev>(ctx, g, run, bitmaps, words,
                                                                                                        grid, counter, dense);
        });
    }
    if (v.sparse()) {
        // the queries of a sparse walk are sparse vectors, or -- the build, which the entry points let through for a mirror
        // of pgv_hnsw_upload_sparse_buildable only -- element slots: then max_q_nnz is the mirror's longest element
        if ((a.sparse_queries.ptr != nullptr) == (a.qids != nullptr))
            PGV_FAIL(PGV_ERR_ARG, "hnsw search: a sparse mirror takes sparse queries, or a build's element slots");
        if (a.max_q_nnz > (a.qids ? kSparseHnswMaxNnz : kSparseMaxNnz))
            PGV_FAIL(PGV_ERR_DIMS, "hnsw search: a query of %d stored elements", a.max_q_nnz);
        if (a.qids) switch (v.metric) {
                case PGV_L2SQ: return launch_hnsw_t<SparseRow, 0, HnswSparse, true>(ctx, g, run, bitmaps, words, grid, counter, sp);
                case PGV_NEG_IP: return launch_hnsw_t<SparseRow, 1, HnswSparse, true>(ctx, g, run, bitmaps, words, grid, counter, sp);
                case PGV_L1: return launch_hnsw_t<SparseRow, 2, HnswSparse, true>(ctx, g, run, bitmaps, words, grid, counter, sp);
                default: PGV_FAIL(PGV_ERR_ARG, "unknown metric %d", (int)v.metric);
            }
        switch (v.metric) {
            case PGV_L2SQ: return launch_hnsw_t<SparseRow, 0>(ctx, g, run, bitmaps, words, grid, counter, sp);
            case PGV_NEG_IP: return launch_hnsw_t<SparseRow, 1>(ctx, g, run, bitmaps, words, grid, counter, sp);
            case PGV_L1: return launch_hnsw_t<SparseRow, 2>(ctx, g, run, bitmaps, words, grid, counter, sp);
        }
        PGV_FAIL(PGV_ERR_ARG, "unknown metric %d", (int)v.metric);
    }
    return dispatch_rows(v, [&](auto *tp, auto mc) {
        return launch_hnsw_t<std::remove_pointer_t<decltype(tp)>, decltype(mc)::value>(ctx, g, run, bitmaps, words, grid, counter);
    });
}

int hnsw_sparse_scan_lds_check(const char *who, pgv_metric metric, int ef, int m, int max_q_nnz) {
    return hnsw_sparse_lds_check(who, ef, m, pad4(max_q_nnz), metric == PGV_NEG_IP ? 0 : bitmap_words(max_q_nnz), true, nullptr);
}

int launch_hnsw_patch(pgv_ctx *ctx, const HnswGraph &graph, int64_t n, const int32_t *ids, const int64_t *packed_off,
                      const int32_t *packed, int nupd) {
    if (nupd <= 0) return PGV_OK;
    hipLaunchKernelGGL(hnsw_patch_kernel, dim3((nupd + 3) / 4), dim3(256), 0, ctx->stream, graph.nbr, graph.nbr_start, n, ids,
                       packed_off, packed, nupd);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

// The (u, v) pairs of every group written out as the slot arrays score_gather_kernel reads (PGV_HNSW_PAIRS_GATHER=1), in
// the order score_groups_kernel writes their values; the groups are described as they are to that kernel.
// One workgroup per group (grid-stride), a row u per step, the row's v spread over the threads (coalesced).
__global__ __launch_bounds__(256) void expand_groups_kernel(const int32_t *__restrict__ ids, const int64_t *__restrict__ ids_at,
                                                            int64_t ids_stride, const int32_t *__restrict__ n_arr,
                                                            const int32_t *__restrict__ from_arr,
                                                            const int64_t *__restrict__ pair_at, int ngroups,
                                                            int32_t *__restrict__ a, int32_t *__restrict__ b) {
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        int64_t at = pair_at[g];
        if (pair_at[g + 1] == at) continue;
        const int64_t i0 = ids_at ? ids_at[g] : (int64_t)g * ids_stride;
        const int n = n_arr ? n_arr[g] : (int)(ids_at[g + 1] - i0);
        const int32_t *gi = ids + i0;
        const int f = from_arr && from_arr[g] > 1 ? from_arr[g] : 1;
        for (int u = f; u < n; u++) {
            const int32_t iu = gi[u];
            for (int v = threadIdx.x; v < u; v += blockDim.x) {
                a[at + v] = iu;
                b[at + v] = gi[v];
            }
            at += u;
        }
    }
}

int launch_expand_groups(pgv_ctx *ctx, const int32_t *ids, const int64_t *ids_at, int64_t ids_stride, const int32_t *n_arr,
                         const int32_t *from_arr, const int64_t *pair_at, int ngroups, int32_t *a, int32_t *b) {
    if (ngroups <= 0) return PGV_OK;
    const int cap = ctx->num_cus * 16;
    hipLaunchKernelGGL(expand_groups_kernel, dim3(ngroups < cap ? ngroups : cap), dim3(256), 0, ctx->stream, ids, ids_at,
                       ids_stride, n_arr, from_arr, pair_at, ngroups, a, b);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

// SelectNeighbors of a batch's new elements (see hnsw_select_kernel): plan -> *out_total_dev pairs at pair_start[ngroups]
int launch_hnsw_select_plan(pgv_ctx *ctx, const int32_t *cnt, int ngroups, int lcap, int m, int64_t *pair_start) {
    if (ngroups <= 0) return PGV_OK;
    hipLaunchKernelGGL(hnsw_select_plan_kernel, dim3(1), dim3(256), 0, ctx->stream, cnt, ngroups, lcap, m, pair_start);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_hnsw_select(pgv_ctx *ctx, const int32_t *lw_ids, const float *lw_dist, const int32_t *cnt, const int32_t *qlevels,
                       const int64_t *pair_start, const float *tri, int ngroups, int lcap, int ef, int m, int stride,
                       int32_t *out_ids, float *out_dist, uint8_t *out_closer, int32_t *out_cnt) {
    if (ngroups <= 0) return PGV_OK;
    static const bool serial = getenv("PGV_HNSW_SELECT_SERIAL") && atoi(getenv("PGV_HNSW_SELECT_SERIAL")) != 0;
    if (ef <= 64 && !serial) {
        hipLaunchKernelGGL(hnsw_select_wave_kernel, dim3((ngroups + 3) / 4), dim3(256), 0, ctx->stream, lw_ids, lw_dist, cnt,
                           qlevels, pair_start, tri, ngroups, lcap, ef, m, stride, out_ids, out_dist, out_closer, out_cnt);
        PGV_HIP(hipGetLastError());
        return PGV_OK;
    }
    hipLaunchKernelGGL(hnsw_select_kernel, dim3((ngroups + 63) / 64), dim3(64), 0, ctx->stream, lw_ids, lw_dist, cnt, qlevels,
                       pair_start, tri, ngroups, lcap, ef, m, stride, out_ids, out_dist, out_closer, out_cnt);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

}  // namespace pgv
