/*
 * pgv_hip.h -- C ABI of libpgv_hip.so: the MI355X (gfx950) implementation of
 * pgvector's distance hot path.
 *
 * This is the drop-in boundary.  pgvector has no batch seam of its own: every
 * distance goes through a per-pair fmgr call (src/ivfflat.h:307 `distfunc`,
 * src/hnswutils.c:524-528 `HnswGetDistance`).  Each entry point below replaces
 * one of the LOOPS around that call; the reference loop it replaces is cited
 * on the declaration.  Host code inside the extension (C)
 * stages vectors out of 8 KB pages into contiguous arrays, calls these
 * functions, and feeds the results back into the same Postgres structures the
 * reference uses (tuplesort, pairing heaps, page writers).
 *
 * Conventions
 *   - plain C: opaque handles, plain pointers and sizes; no C++/torch types.
 *   - every function returns PGV_OK or a PGV_ERR_* code; the message of the
 *     last failure on the calling thread is pgv_last_error().
 *   - buffer arguments may be HOST or DEVICE pointers; the library asks the HIP
 *     runtime which (hipPointerGetAttributes) and stages host buffers through
 *     its own pinned/device scratch.  A Postgres backend passes host memory; a
 *     harness that already keeps data in HBM passes device memory and pays no
 *     PCIe traffic.
 *   - a handle is used by one thread at a time (a Postgres backend is single
 *     threaded); different handles may be used concurrently.
 *   - all work is enqueued on the context's HIP stream; functions that return
 *     results into host memory synchronise that stream before returning,
 *     functions whose outputs are device pointers do not (pgv_ctx_sync does).
 *   - vectors are `dim` consecutive elements of `dtype` (float or IEEE
 *     binary16), row-major, densely packed: the payload of the reference's
 *     Vector / HalfVector varlenas (src/vector.h:18-24, src/halfvec.h:68-74)
 *     without the 8-byte header.
 *   - distances come back as the fp32 value of the reference's kernel
 *     (src/vector.c:560-617, src/halfutils.c:29-121); the float8 widening,
 *     sqrt, negation-for-display etc. of the fmgr wrappers is exact host work.
 *   - there is NO CPU fallback: without a usable gfx950 device every call
 *     fails with PGV_ERR_DEVICE.
 */
#ifndef PGV_HIP_H
#define PGV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGV_ABI_VERSION 1

/* status codes */
#define PGV_OK 0
#define PGV_ERR_ARG 1			/* bad argument (NULL, negative size, ...) */
#define PGV_ERR_DIMS 2			/* dimension limits: 1..16000 (src/vector.h:10) */
#define PGV_ERR_DEVICE 3		/* no usable GPU / HIP runtime error */
#define PGV_ERR_NOMEM 4			/* device or host allocation failed */
#define PGV_ERR_STATE 5			/* handle in the wrong state */
#define PGV_ERR_DATA 6			/* data error the reference would elog (NaN center, ...) */

/* element type of an indexed column: vector (float4) or halfvec (binary16) */
typedef enum pgv_dtype
{
	PGV_F32 = 0,
	PGV_F16 = 1
}			pgv_dtype;

/*
 * Distance computed by a kernel = FUNCTION 1 of the operator class
 * (src/ivfflat.h:40 IVFFLAT_DISTANCE_PROC, src/hnsw.h:37 HNSW_DISTANCE_PROC):
 *   PGV_L2SQ    vector_l2_squared_distance / halfvec_l2_squared_distance   (sql/vector.sql:409,822)
 *   PGV_NEG_IP  vector_negative_inner_product / halfvec_...                (sql/vector.sql:415,422,828,835)
 *   PGV_L1      l1_distance (hnsw vector_l1_ops, sql/vector.sql:445)
 */
typedef enum pgv_metric
{
	PGV_L2SQ = 0,
	PGV_NEG_IP = 1,
	PGV_L1 = 2
}			pgv_metric;

/*
 * Operator-class family, for the build path where FUNCTION 3/4 matter too:
 *   PGV_OPS_L2      k-means on l2_distance, nothing normalised
 *   PGV_OPS_IP      spherical k-means (samples and centers normalised), rows stored as-is
 *   PGV_OPS_COSINE  spherical k-means, rows stored normalised, zero rows skipped
 * (sql/vector.sql:406-425; src/ivfbuild.c:69-73,154-155,174-180)
 */
typedef enum pgv_ops
{
	PGV_OPS_L2 = 0,
	PGV_OPS_IP = 1,
	PGV_OPS_COSINE = 2
}			pgv_ops;

typedef struct pgv_ctx pgv_ctx;		/* one GPU + stream + scratch */
typedef struct pgv_index pgv_index;	/* device mirror of one IVFFlat index */
typedef struct pgv_hnsw pgv_hnsw;	/* device mirror of one HNSW index's element vectors */

/*
 * Source of RandomDouble()/RandomInt() (src/ivfflat.h:86-94).  Inside Postgres
 * the callbacks wrap pg_prng_double/pg_prng_uint32 on pg_global_prng_state so
 * the stream of draws is the reference's.  NULL callbacks select the library's
 * own xoroshiro128** seeded with `seed`.
 */
typedef struct pgv_rng
{
	double		(*next_double) (void *state);	/* uniform [0,1) */
	uint32_t	(*next_u32) (void *state);
	void	   *state;
	uint64_t	seed;
}			pgv_rng;

/* ------------------------------------------------------------------ context */

const char *pgv_last_error(void);
int			pgv_abi_version(void);

/* number of HIP devices visible (0 when there is no GPU / no driver) */
int			pgv_device_count(void);
/*
 * Products per accumulator chain that the deterministic rounding band of the matrix-core L2 paths charges for rows of
 * `dim` elements (ScanBound's g_dot = gamma_(chain + 4)): path 0 the list scan and center ranking on the 32-query
 * kernel, 1 the list scan on the 64-query kernel, 2 pgv_exact_topk's 128 x 128 tiling.  For tests and diagnostics;
 * needs no device.  -1: unknown dtype / path.
 */
int			pgv_scan_chain_length(int dim, pgv_dtype dtype, int path);
/* free / total HBM of a device in bytes as the driver reports them now (all processes' allocations counted) */
int			pgv_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);
/*
 * Page-locked host memory (hipHostMalloc) for buffers handed to the library again and again -- the lanes of
 * the host glue's pooler (pgv_host_pool_*), a backend's query staging.  Plain host memory works everywhere
 * too; pinned memory makes the copies in and out asynchronous and about twice as fast.
 */
int			pgv_pinned_alloc(size_t bytes, void **out);
void		pgv_pinned_free(void *p);
/*
 * Page-lock memory the caller already owns -- a range of a shared-memory segment (Postgres' DSM / the main shared
 * memory block) that several processes fill and the process that owns the GPU context hands to the library: the
 * pooler's query and result lanes (pgv_host_pool_*).  Registration is per process and optional: an unregistered
 * range is staged through the library's own pinned scratch.
 */
int			pgv_pinned_register(void *p, size_t bytes);
void		pgv_pinned_unregister(void *p);

/*
 * Create the per-backend GPU context: lazily from _PG_init (src/vector.c:57-65)
 * or on first use.  `stream` is an existing hipStream_t to enqueue on (as
 * void*), PGV_DEFAULT_STREAM for the device's default stream (whose handle is
 * itself NULL), or NULL to create a private non-blocking stream.  A caller that
 * produces inputs / consumes outputs in HBM on its own stream must pass that
 * stream, or bracket calls with its own synchronisation.
 */
#define PGV_DEFAULT_STREAM ((void *) (intptr_t) -1)	/* the device's default (NULL) hipStream_t */
int			pgv_ctx_create(int device, void *stream, pgv_ctx * *out);
void		pgv_ctx_destroy(pgv_ctx * ctx);
int			pgv_ctx_sync(pgv_ctx * ctx);
/* the hipStream_t all work of this context is enqueued on */
void	   *pgv_ctx_stream(pgv_ctx * ctx);
/* time the enclosed GPU work with HIP events on the context's stream (ms) */
int			pgv_timer_start(pgv_ctx * ctx);
int			pgv_timer_stop(pgv_ctx * ctx, float *out_ms);

/*
 * Optional per-kernel accounting for the roofline report: when on, every
 * launch of the row-streaming distance kernel is bracketed by HIP events on the
 * context's stream; pgv_ctx_get_stats synchronises, resolves them and returns
 * the totals since the last pgv_ctx_reset_stats.
 */
typedef struct pgv_stats
{
	/* the IVFFlat list scan (GetScanItems): pgv_scan_lists / pgv_search_batch */
	double		scan_ms;		/* GPU time inside the row-streaming kernel */
	int64_t		scan_launches;
	double		scan_pairs;		/* (row, query) distances it produced */
	double		scan_rows;		/* rows it streamed (a row shared by a query group counts once) */
	/* the same kernel on other inputs: center ranking, exact scans, k-means++ rounds */
	double		aux_ms;
	int64_t		aux_launches;
	double		aux_pairs;
	/* L2 assignment on the matrix cores (pgv_assign / k-means): rows it handled, how many of them the
	 * pre-filter left to the exact recheck of its 4 candidates, and how many the exact kernel redid in full */
	double		assign_redo_rows;
	double		assign_rows;
	double		assign_recheck_rows;
	/* batched list scans: rows of the lists at least one query of the batch probes -- what a single pass
	 * over the probed part of the index would stream (scan_rows / scan_unique_rows = passes) */
	double		scan_unique_rows;
	/* L2 batches scanned on the matrix cores: queries whose k' candidates could not be proven to hold
	 * the whole head and took the exact pass over their segment as well.  The batch's center ranking
	 * (pgv_rank_lists / pgv_search_batch: maxprobes + 16 candidates of the centers, on the fp16 center
	 * shadow where the index has one) counts here too: a query appears once per half that flagged it */
	double		scan_redo_queries;
	/* ... and those that a wider candidate set (256 instead of k') did settle, without the exact pass
	 * (list scan and center ranking alike) */
	double		scan_widened_queries;
	/* batches over the fp16 residual shadow: probed (query, list) pairs that were not scanned because every
	 * row of the list is provably farther than k rows of the lists probed before it (PGV_PROBE_PRUNE) */
	double		scan_pruned_probes;
	/* fp32 L2 batches scanned on the matrix cores: queries whose pre-filter read the fp16 residual shadow
	 * of the index instead of its fp32 rows (counted whether or not profiling is on) */
	double		scan_shadow_queries;
}			pgv_stats;
int			pgv_ctx_set_profiling(pgv_ctx * ctx, int on);
/*
 * The batched list scan (pgv_search_batch / pgv_scan_batch) picks L2 candidates with the matrix cores'
 * |q|^2 + |x|^2 - 2 q.x and then evaluates the reference's sum((q - x)^2) for those only; results are the
 * same as evaluating every row exactly.  on != 0 keeps every row on the exact vector-ALU kernels (A/B
 * measurements, and indexes whose rows mix magnitudes so widely that every query would be redone).
 */
int			pgv_ctx_set_exact_scan(pgv_ctx * ctx, int on);
/*
 * How the MFMA L2 paths (batched list scan, center ranking, assignment pre-filter, pgv_exact_topk) bound the
 * distance between the expansion's value |x|^2 - 2 q.x and the true one when they decide that a candidate set is
 * complete.  Row ids "must match the reference CPU path": with either bound every decision the bound cannot settle
 * goes to the exact kernels; what differs is whether the bound itself can be exceeded.
 *   PGV_BOUND_WORST_CASE (default)  deterministic: the list scan keeps FOUR independent accumulator chains per output,
 *       so its dot product errs by at most gamma_(dim/4 + 4) |q||x| (Higham, Lemma 3.1: any order of n rounded
 *       products), gamma_n = n u / (1 - n u) with u = 2^-24 (the matrix pipeline rounds to nearest: pinned on the
 *       hardware by tests/test_gpu_round4.py); + the row norm's own chain; + the rounding of the exact form
 *       sum((q - x)^2) -- the reference's and ours -- which is relative to the DISTANCE, not to (|q| + |x|)^2.  At 1536
 *       dimensions: 2.3e-5 x 2 |q||x|max, narrower than the statistical band, which is why it can be the default (bench.py `bound_modes`: both side by side; round 3's form of it,
 *       (gamma_(dim+1) + gamma_(dim+2)) (|q| + |x|max)^2 on one chain, flagged every query and cost 98 %).
 *   PGV_BOUND_STATISTICAL  8 sqrt(dim + 4) 2^-24 (|q| + |x|max)^2 -- the probabilistic model of a length-dim fp32
 *       summation (fails with probability ~ e^-32 per sum).
 * A context starts with the deterministic bound EVERYWHERE (round 6), the build's assignment pre-filter included.  That
 * kernel has one accumulator chain per output (128 accumulators a lane leave no room for four), so its band is
 * gamma_(dim+1) (|c|^2 + 2 |a||c|) + gamma_(dim+2) d, 5-10 x wider than the statistical one; what makes it affordable is
 * that an ambiguous row costs an exact recheck of the candidates inside the band (a row's merged list carries 8 of them
 * and the smallest value no list kept) instead of a pass over all centers: +4 % at 1 M x 1000 x 1536 fp32, +10 % at
 * 1.25 M x 4096 x 3072 fp16 over the statistical bound (round 5's form of it: 32 -> 123 ms).  pgv_ctx_set_bound(mode)
 * sets scans and assignment alike.
 * pgv_ctx_set_exact_scan(ctx, 1) remains the mode that uses no expansion at all.
 */
#define PGV_BOUND_STATISTICAL 0
#define PGV_BOUND_WORST_CASE 1
int			pgv_ctx_set_bound(pgv_ctx * ctx, int mode);
int			pgv_ctx_reset_stats(pgv_ctx * ctx);
int			pgv_ctx_get_stats(pgv_ctx * ctx, pgv_stats * out);

/* ------------------------------------------------------- IVFFlat scan side */

/*
 * Upload (or adopt, when the pointers are device memory the index is copied
 * device-to-device) a list-major image of an IVFFlat index:
 *   centers       [nlists x dim]   the Vector inside each IvfflatListData (src/ivfflat.h:270-275)
 *   list_offsets  [nlists + 1]     row range of list l = [off[l], off[l+1]) -- its page chain, flattened
 *   vectors       [n x dim]        index tuple payloads in page-chain order (src/ivfscan.c:139-179)
 *   tids          [n] or NULL      heap TIDs (ItemPointerData widened to 64 bit); NULL -> results carry row slots
 * Replaces the ReadBuffer/LockBuffer page walks of GetScanLists/GetScanItems.
 */
int			pgv_index_upload(pgv_ctx * ctx, pgv_metric metric, pgv_dtype dtype, int dim, int nlists,
							 const void *centers, const int64_t *list_offsets,
							 const void *vectors, const uint64_t *tids, pgv_index * *out);
void		pgv_index_free(pgv_index * index);
/*
 * A second handle on an uploaded index for another context (= another backend's stream and scratch) on the same
 * device: many backends scan ONE device mirror concurrently, each on its own stream -- what shared_buffers is to
 * the reference's scans.  The index is read-only after upload, so no locking is involved.  The handles share the
 * device arrays, which are released by the last pgv_index_free among them (in any order).
 */
int			pgv_index_share(pgv_index * index, pgv_ctx * ctx, pgv_index * *out);
/*
 * Overlapping batches.  A batch of pgv_search_batch is ~25 dependent launches on one stream: center ranking, planning,
 * the list scan (which streams the probed lists once and is HBM-bound), top-k, exact recheck.  Two submitters on two
 * contexts already overlap one batch's ranking / planning / top-k with the other's scan (the scans themselves cannot
 * overlap: both want the whole HBM); lanes > 1 gives ONE caller the same: consecutive pgv_search_batch calls on this
 * handle run on `lanes` internal streams in turn (each with scratch of its own; the index stays one).  With lanes > 1
 *   - a call returns when its work is enqueued; device-side outputs are complete after pgv_ctx_sync(the index's
 *     context) (which waits for the lanes too), NOT merely in the order of that context's stream;
 *   - device-side queries are read no earlier than what the context's stream held at the call (an event orders it);
 *   - host-side outputs make the call synchronous, as always (nothing overlaps then);
 *   - statistics, profiling and the bound / exact-scan settings of the context include the lanes.
 * lanes = 1 (the default) restores the stream-ordered behaviour.  Views (pgv_index_share / _import) have lanes of their
 * own or none.  1 <= lanes <= 4.
 */
int			pgv_index_set_overlap(pgv_index * index, int lanes);
/*
 * The same across PROCESSES -- a Postgres backend is a process (src/ivfscan.c:252-296 runs in each), and its parallel
 * build shares state through a DSM segment (src/ivfbuild.c:830-966).  The whole mirror (centers, vectors, offsets,
 * TIDs, norms) is one device allocation; pgv_index_export wraps its hipIpcMemHandle and the mirror's shape into a
 * fixed-size, position-independent handle that the owner publishes in shared memory; every other process maps the
 * SAME HBM with pgv_index_import and scans it on its own context (stream + scratch).  The index occupies HBM once,
 * whatever the number of backends.
 *   - the exporting process must keep its index (and itself) alive while others have it mapped: inside the server
 *     that is the background worker that staged the index, not a backend that may exit;
 *   - an importer releases its mapping with pgv_index_free; a handle cannot be imported by the process that
 *     exported it (PGV_ERR_STATE: that process uses pgv_index_share);
 *   - the ROCm driver shares memory through dmabuf here: HSA_ENABLE_IPC_MODE_LEGACY=0 in every process.
 */
#define PGV_INDEX_HANDLE_BYTES 256
typedef struct pgv_index_handle
{
	unsigned char bytes[PGV_INDEX_HANDLE_BYTES];
}			pgv_index_handle;
int			pgv_index_export(pgv_index * index, pgv_index_handle * out);
int			pgv_index_import(pgv_ctx * ctx, const pgv_index_handle * handle, pgv_index * *out);
/*
 * Heap TIDs of row slots (what pgv_scan_lists hands back), for a caller that keeps no TID table of its own -- a
 * backend that imported the mirror.  slots / out are host arrays; runs of consecutive slots (a list) are one copy.
 */
int			pgv_index_tids(pgv_index * index, const int64_t *slots, int64_t n, uint64_t *out);
int64_t		pgv_index_rows(const pgv_index * index);
int			pgv_index_lists(const pgv_index * index);

/*
 * GetScanLists (src/ivfscan.c:47-118) for a batch of queries: distance from each
 * query to every center, keep the `maxprobes` nearest, ascending.  Ties on the
 * boundary keep the lower list id (the reference's strict `<` at :92).
 *   queries    [nq x dim]
 *   out_lists  [nq x maxprobes] list ids (maxprobes is clamped to nlists by the caller, :271-278)
 *   out_dist   [nq x maxprobes] or NULL
 */
int			pgv_rank_lists(pgv_index * index, const void *queries, int nq, int maxprobes,
						   int32_t *out_lists, float *out_dist);

/*
 * GetScanItems (src/ivfscan.c:123-187) without the final sort: the distance of
 * every tuple of the given lists to one query, in the order the reference
 * feeds its tuplesort (lists in the given order, page-chain order inside).
 *   out_dist  [m]  m = sum of the list lengths (query NULL -> all 0: ZeroDistance :192-196)
 *   out_slot  [m]  row slot of each tuple (index into vectors/tids)
 *   capacity  size of the out arrays; *out_count = m (PGV_ERR_ARG if m > capacity)
 * The caller widens to float8 and runs the same tuplesort as the reference.
 */
int			pgv_scan_lists(pgv_index * index, const void *query, const int32_t *lists, int nlists,
						   float *out_dist, int64_t *out_slot, int64_t capacity, int64_t *out_count);

/*
 * Fused query path for many backends' queries at once: GetScanLists +
 * GetScanItems + the head of the sorted tuplesort stream (src/ivfscan.c:360-414),
 * i.e. for each query the k nearest tuples of its `probes` nearest lists,
 * ascending (ties: lower insertion position first).
 *   out_dist  [nq x k]   +inf padded when fewer than k tuples were scanned
 *   out_slot  [nq x k]   row slots, -1 padded
 *   out_tid   [nq x k]   or NULL; heap TIDs when the index was uploaded with tids
 */
int			pgv_search_batch(pgv_index * index, const void *queries, int nq, int probes, int k,
							 float *out_dist, int64_t *out_slot, uint64_t *out_tid);

/*
 * The query cast of the fp16 shadow paths on its own, for tests: what pgv_search_batch prepares once per batch for an
 * fp32 L2 index that has its fp16 shadows (PGV_ERR_STATE otherwise).  out_qcast [nq x ld16] fp16 bits, ld16 = dim
 * rounded up to 8: the queries times 2^-s_q, s_q per query; out_qscale / out_qeps [nq]: the list scan's factor
 * 2^(1 + s + s_q) and the query's term of its rounding band; out_cscale / out_ceps [nq]: the same for the center
 * ranking.  Any output may be NULL.  Host or device pointers; complete on return.
 */
int			pgv_index_shadow_cast(pgv_index * index, const void *queries, int nq, void *out_qcast, float *out_qscale,
								  float *out_qeps, float *out_cscale, float *out_ceps);

/*
 * The GetScanItems half of pgv_search_batch on its own: the probe lists were chosen
 * elsewhere (pgv_rank_lists, possibly on another GPU: with the index sharded by list,
 * every rank ranks a slice of the queries against the replicated centers, the probe lists
 * are all-gathered, and each rank scans the lists it owns).  Lists that are empty in this
 * image contribute nothing.
 *   probe_lists [nq x probes] list ids, ascending by distance per query
 */
int			pgv_scan_batch(pgv_index * index, const void *queries, int nq, const int32_t *probe_lists,
						   int probes, int k, float *out_dist, int64_t *out_slot, uint64_t *out_tid);

/*
 * One backend's index scan, device-resident between the amgettuple calls (src/ivfscan.c:361-414).
 * This is the path a Postgres backend binds: one query at a time, LIMIT k tuples pulled.
 *   pgv_query_rank   GetScanLists (src/ivfscan.c:47-118): ranks every center against the query
 *                    and keeps the max_probes nearest ON THE DEVICE (one launch, nothing read back).
 *                    query NULL = ZeroDistance (:192-196): lists 0 .. max_probes-1.
 *   pgv_query_scan   GetScanItems + tuplesort_performsort (:123-187) for ranked lists
 *                    [first, first + nprobes): every tuple scored (one launch, the rows spread over
 *                    all CUs), the distances stay in HBM in tuplesort input order, and only the
 *                    `head` nearest come back, ascending (ties: lower insertion position first):
 *                    out_dist / out_slot / out_tid [head], *out_count = min(head, tuples),
 *                    *out_total = tuples in the batch (what the reference's tuplesort holds).
 *   pgv_query_more   entries [skip, skip + count) of the same batch's sorted stream, for an
 *                    executor that pulls past the head; skip + count <= 1024.  Beyond that the
 *                    caller fetches the whole batch with pgv_scan_lists (pgv_query_lists gives the
 *                    ranked list ids) and sorts it like the reference does.
 * Limits of the fused path: max_probes <= 1024, nprobes <= 256, head <= 1024 (PGV_ERR_ARG
 * otherwise: use pgv_rank_lists / pgv_scan_lists).  Iterative scans (:400-406) call
 * pgv_query_scan again with first += nprobes.  out_tid needs an index uploaded with tids.
 */
typedef struct pgv_query pgv_query;
int			pgv_query_begin(pgv_index * index, pgv_query * *out);
void		pgv_query_end(pgv_query * q);
int			pgv_query_rank(pgv_query * q, const void *query, int max_probes);
int			pgv_query_scan(pgv_query * q, int first, int nprobes, int head, float *out_dist, int64_t *out_slot,
						   uint64_t *out_tid, int *out_count, int64_t *out_total);
int			pgv_query_more(pgv_query * q, int skip, int count, float *out_dist, int64_t *out_slot,
						   uint64_t *out_tid, int *out_count);
int			pgv_query_lists(pgv_query * q, int32_t *out_lists, int n);

/* ------------------------------------------------------ IVFFlat build side */

/*
 * The argmin loop of AddTupleToSort (src/ivfbuild.c:183-192) for a batch of
 * heap rows: list id of the nearest center under FUNCTION 1, first
 * strictly-smallest wins.
 *   centers [k x dim], rows [n x dim], out_list [n], out_dist [n] or NULL
 */
int			pgv_assign(pgv_ctx * ctx, pgv_metric metric, pgv_dtype dtype, int dim,
					   const void *centers, int k, const void *rows, int64_t n,
					   int32_t *out_list, float *out_dist);

/*
 * IvfflatKmeans (src/ivfkmeans.c:553-570): k-means++ seeding (:23-91) followed
 * by Lloyd iterations to the reference's stopping rule (:347, :482-483), new
 * centers as fp32 sums in sample order / count (:179-236), empty clusters
 * refilled from the rng (:222-227), spherical variant for ip/cosine (:234-235),
 * CheckCenters (:490-547).  Elkan's bounds (:391-476) are a CPU-side pruning of
 * exactly this computation and are not reproduced: every sample is scored
 * against every center each iteration.
 *   samples      [n x dim] as left by SampleRows (already normalised for ip/cosine, src/ivfbuild.c:154-155)
 *   out_centers  [k x dim] in `dtype`
 *   out_closest  [n] final assignment, or NULL
 *   out_iters    iterations run, or NULL
 * n == 0 -> RandomCenters (:110-133).
 */
int			pgv_kmeans(pgv_ctx * ctx, pgv_ops ops, pgv_dtype dtype, int dim,
					   const void *samples, int n, int k, int max_iterations, const pgv_rng * rng,
					   void *out_centers, int32_t *out_closest, int *out_iters);

/*
 * The two halves of one Lloyd iteration, exposed so that a multi-GPU build can
 * put its all-reduce between them (samples sharded by row, centers replicated):
 *   pgv_lloyd_partial: assignment of this rank's samples to `centers` + this
 *       rank's per-center fp32 sums [k x dim], counts [k] and the number of
 *       samples whose center changed versus io_closest (updated in place).
 *   pgv_lloyd_finish:  centers = sums / counts (inf clamp, empty -> rng, dtype
 *       rounding, renormalise) from the all-reduced sums/counts.
 * All pointers follow the host-or-device rule; with device pointers nothing
 * synchronises, so RCCL can be enqueued on the same stream in between.
 */
int			pgv_lloyd_partial(pgv_ctx * ctx, pgv_ops ops, pgv_dtype dtype, int dim,
							  const void *samples, int n, const void *centers, int k,
							  int32_t *io_closest, float *out_sums, int32_t *out_counts,
							  int64_t *out_changes);
int			pgv_lloyd_finish(pgv_ctx * ctx, pgv_ops ops, pgv_dtype dtype, int dim, int k,
							 const float *sums, const int32_t *counts, const pgv_rng * rng,
							 void *out_centers);

/*
 * InitCenters (src/ivfkmeans.c:23-91) alone: k-means++ seeding under the
 * FUNCTION 3 distance.  out_centers [k x dim].
 */
int			pgv_kmeanspp_init(pgv_ctx * ctx, pgv_ops ops, pgv_dtype dtype, int dim,
							  const void *samples, int n, int k, const pgv_rng * rng,
							  void *out_centers);

/* ------------------------------------------- multi-GPU: one process per GPU */

/*
 * IVFFlat shards naturally: k-means samples and heap rows by row, lists by l % nranks,
 * centers replicated.  The exchange steps of the path live HERE, in the library, enqueued on the
 * context's stream between the kernels that produce and consume their buffers (the reference runs
 * its parallel build inside the extension too, src/ivfbuild.c:830-966):
 *   k-means     per k-means++ round one all-gather of the ranks' weight totals and one of the candidate
 *               rows; per Lloyd iteration ONE all-reduce of sums [k x dim] | counts [k] | changes as a
 *               single fp32 buffer (k*d*4 + k*4 + 4 bytes), no host synchronisation: the host follows
 *               the iteration through a 24-byte record in pinned memory
 *   list scan   all-gather of the probe lists every rank chose for its slice of the query batch, and
 *               of every rank's k x (distance, tid) per query, merged on the device
 * pgv_comm_create uses RCCL over xGMI (librccl is resolved at run time; nothing is linked).
 * pgv_comm_create_custom takes the two collectives from the caller instead -- a Postgres parallel
 * build can back them with its DSM segment, the CPU-side tests with gloo.
 * HNSW search does not shard: replicas only.
 */
typedef struct pgv_comm pgv_comm;

#define PGV_COMM_ID_BYTES 128
/* rank 0 makes the id of a new group (ncclGetUniqueId); the host hands it to every rank by whatever channel it has */
int			pgv_comm_unique_id(void *out_id);
int			pgv_comm_create(pgv_ctx * ctx, int nranks, int rank, const void *unique_id, pgv_comm * *out);

/* both operate on DEVICE buffers and must be ordered after the work already enqueued on `stream` and
 * before whatever is enqueued next (a host implementation synchronises the stream on entry) */
typedef struct pgv_collectives
{
	int			(*all_reduce_sum_f32) (void *state, float *buf, size_t count, void *stream);	/* in place */
	int			(*all_gather) (void *state, const void *send, void *recv, size_t bytes_per_rank, void *stream);
	void	   *state;
}			pgv_collectives;
int			pgv_comm_create_custom(pgv_ctx * ctx, int nranks, int rank, const pgv_collectives * coll, pgv_comm * *out);
void		pgv_comm_destroy(pgv_comm * comm);
int			pgv_comm_size(const pgv_comm * comm);
int			pgv_comm_rank(const pgv_comm * comm);

/*
 * pgv_kmeans with the samples sharded by row: samples_local [n_local x dim] are this rank's rows of the
 * sample (global order = rank order), every rank gets the same centers.  Every rank must pass the same
 * rng stream (seed or callbacks in the same state): the draws steer replicated decisions.
 *   out_centers [k x dim], out_closest_local [n_local] or NULL
 */
int			pgv_kmeans_sharded(pgv_comm * comm, pgv_ops ops, pgv_dtype dtype, int dim,
							   const void *samples_local, int n_local, int k, int max_iterations,
							   const pgv_rng * rng, void *out_centers, int32_t *out_closest_local, int *out_iters);

/*
 * pgv_search_batch over an index whose lists are sharded l % nranks (`local_index` holds all list
 * offsets, foreign lists empty, replicated centers, and was uploaded with tids): every rank passes the
 * SAME batch of nq queries, ranks its slice of it against the centers, scans the probed lists it owns
 * for all of them, and ends up with the merged k nearest (distance, tid) of every query.
 *   out_dist [nq x k], out_tid [nq x k]  (ties: lower rank first)
 */
int			pgv_search_batch_sharded(pgv_comm * comm, pgv_index * local_index, const void *queries, int nq,
									 int probes, int k, float *out_dist, uint64_t *out_tid);

/*
 * The build's tuplesort on the device.  The reference's BuildCallback assigns every heap row to its nearest center
 * and feeds (list, tid, vector) to a tuplesort ordered by list (AddTupleToSort src/ivfbuild.c:161-219, the sort
 * :606-615); InsertTuples (:271-331) then walks the sorted stream list by list into pages.  With the rows in HBM
 * anyway (pgv_assign staged them), the sort is a device gather and its result IS the device mirror:
 *
 *   pgv_builder_begin   centers of the index (after IvfflatKmeans); expected_rows sizes the first allocation.
 *                       centers == NULL: they come later -- until pgv_builder_set_centers, pgv_builder_add only copies
 *                       its rows to the device, on a stream of the builder's own, so that the upload of the heap and a
 *                       pgv_kmeans still running on the context (called from another host thread) overlap; the rows
 *                       are assigned in one piece once the centers are there.  (That stream is not ordered after the
 *                       context's: device-resident rows handed to such a builder must be complete before the call.)
 *   pgv_builder_add     a batch of heap rows (host or device, tightly packed) with their TIDs (or NULL: heap
 *                       positions): copied to the device, assigned there (same kernel as pgv_assign), kept in heap order
 *   pgv_builder_finish  list-major order (ascending list, heap order inside a list -- what the tuplesort delivers
 *                       to InsertTuples), the mirror made from it without a second upload; out_offsets [lists + 1]
 *                       and out_lists [rows, heap order] (either may be NULL) go back to the host
 *   pgv_index_drain     the mirror's rows in list-major order, piece by piece through pinned memory (the next
 *                       piece's copy in flight while the sink runs): what the page writer consumes
 *
 * The builder holds the heap-order copy until finish (2 x the rows in HBM for a moment: 12 GB at 1 M x 1536).
 */
typedef struct pgv_builder pgv_builder;
int			pgv_builder_begin(pgv_ctx * ctx, pgv_metric metric, pgv_dtype dtype, int dim, int nlists, const void *centers,
							  int64_t expected_rows, pgv_builder * *out);
int			pgv_builder_add(pgv_builder * b, const void *rows, const uint64_t *tids, int64_t n);
/* the centers of a builder begun without them (PGV_ERR_STATE otherwise); called once, before pgv_builder_finish */
int			pgv_builder_set_centers(pgv_builder * b, const void *centers);
int64_t		pgv_builder_rows(const pgv_builder * b);
int			pgv_builder_finish(pgv_builder * b, pgv_index * *out_index, int64_t *out_offsets, int32_t *out_lists);
void		pgv_builder_free(pgv_builder * b);
/* sink(arg, first_slot, count, vectors [count x dim] tightly packed, tids [count] or NULL) -> 0 to go on */
typedef int (*pgv_rows_sink) (void *arg, int64_t first_slot, int64_t count, const void *vectors, const uint64_t *tids);
int			pgv_index_drain(pgv_index * index, int64_t chunk_rows, pgv_rows_sink sink, void *arg);

/* ------------------------------------------------- generic candidate batch */

/*
 * One query against n contiguous rows: the exact-scan shape (one fmgr call
 * per heap row, src/vector.c:579-589) and the building block of HNSW candidate
 * scoring.  out[n] = kernel value (L2 squared / -ip / L1).
 */
int			pgv_distance_batch(pgv_ctx * ctx, pgv_metric metric, pgv_dtype dtype, int dim,
							   const void *query, const void *rows, int64_t n, float *out);

/*
 * The exact scan for a BATCH of queries: `ORDER BY embedding <op> $1 LIMIT k` without an index is one fmgr call per
 * heap row (l2_distance src/vector.c:579-589, vector_negative_inner_product :610-620, l1_distance :715-725; the
 * halfvec twins src/halfvec.c:605-748) feeding the executor's top-N heapsort.  nq queries against the same n rows:
 * out_dist [nq x k] ascending kernel values (L2 squared / -ip / L1: the sqrt and the sign stay float8 post-ops of
 * the caller, both monotonic), out_idx [nq x k] row indexes, ties by lower index; entries beyond n are +inf / -1.
 * queries / rows / outputs may be host or device memory.  L2 and inner product batches of 64 queries or more run on
 * the matrix cores (L2 with the exact tail of the list scan, see pgv_ctx_set_bound), everything else on the exact
 * vector-ALU kernels.  k <= 4096.
 */
int			pgv_exact_topk(pgv_ctx * ctx, pgv_metric metric, pgv_dtype dtype, int dim, const void *queries, int nq,
						   const void *rows, int64_t n, int k, float *out_dist, int64_t *out_idx);

/*
 * cosine_distance as the operator computes it without an index (`<=>` in a sequential scan or an
 * executor recheck; src/vector.c:649-697, src/halfvec.c:652-700): three fp32 accumulators in one
 * pass, `(double) sim / sqrt((double) na * (double) nb)`, clamped to [-1, 1], 1 - similarity.  A
 * zero vector gives NaN like the reference (test/expected/vector_type.out:437-441).  out [n] float8.
 */
int			pgv_cosine_distance_batch(pgv_ctx * ctx, pgv_dtype dtype, int dim,
									  const void *query, const void *rows, int64_t n, double *out);

/*
 * hamming_distance / jaccard_distance (`<~>`, `<%>`; src/bitvec.c:45-70 over src/bitutils.c:49-131)
 * of one bit string against n bit strings of the same length: VARBITS payloads, (nbits + 7) / 8
 * bytes each, first bit = most significant bit of byte 0, rows contiguous.  out [n] float8 (exact).
 */
typedef enum pgv_bit_metric
{
	PGV_BIT_HAMMING = 0,
	PGV_BIT_JACCARD = 1
}			pgv_bit_metric;

int			pgv_bit_distance_batch(pgv_ctx * ctx, pgv_bit_metric metric, int nbits,
								   const void *query, const void *rows, int64_t n, double *out);

/*
 * `ORDER BY b <~> $1 LIMIT k` without an index, for a BATCH of queries (hamming_distance src/bitvec.c:45-56 over
 * BitHammingDistanceDefault src/bitutils.c:49-73, feeding the executor's top-N sort): the first stage of the
 * binary-quantization query of the reference's README.  queries [nq x bytes] and rows [n x bytes], bytes =
 * (nbits + 7) / 8: VARBITS payloads as pgv_bit_distance_batch takes them, contiguous, first bit = most significant bit
 * of byte 0; bytes are counted whole like the reference does, so the caller's pad bits are zero (as PostgreSQL keeps
 * them).  out_dist [nq x k] Hamming distances ascending, as floats (exact: at most 512 000), out_idx [nq x k] row
 * indexes, ties by lower index (pgv_exact_topk's rule); entries beyond n are +inf / -1.  Every array may be host or
 * device memory; device rows whose byte length is a multiple of 16 are used in place.  1 <= k <= 4096,
 * 0 <= nbits <= 512 000 (nbits == 0: every distance is 0, the answer is rows 0 .. min(k, n) - 1), n <= 2^32.  The
 * queries are served in chunks of min(nq, max(1, 2^30 / n)) (whole multiples of 32 from 32 on), so that a chunk's
 * distance matrix stays at or under 2^30 floats.
 */
int			pgv_bit_topk(pgv_ctx * ctx, int nbits, const void *queries, int nq,
						 const void *rows, int64_t n, int k, float *out_dist, int64_t *out_idx);

/*
 * binary_quantize (src/vector.c:952-979, halfvec_binary_quantize in src/halfvec.c): bit i = x[i] > 0, exactly the C
 * comparison -- +0.0, -0.0, NaN and negatives give 0, every positive value 1 (+inf and the subnormals included; the
 * bit is decided from the element's pattern, not by a floating-point compare).  rows [n x dim] host or device,
 * out_bits [n x (dim + 7) / 8] bytes host or device, packed contiguous, first element in the most significant bit of
 * byte 0, the unused low bits of a row's last byte zero: what pgv_bit_topk reads.
 */
int			pgv_binary_quantize(pgv_ctx * ctx, pgv_dtype dtype, int dim, const void *rows, int64_t n, void *out_bits);

/*
 * The outer ORDER BY of the two-stage query (`ORDER BY embedding <=> $1 LIMIT k` over the subquery's rows: one
 * l2_distance / vector_negative_inner_product / l1_distance call per surviving row, src/vector.c:579-725, halfvec
 * twins src/halfvec.c:605-748): exact kernel values of each query against ITS candidates only.
 *   rows [n x dim], queries [nq x dim], cand [nq x kc] row indexes (-1 = none), k <= kc <= 4096, n < 2^31
 *   out_dist [nq x k] ascending kernel values (L2 squared / -ip / L1, like pgv_exact_topk), out_idx [nq x k] row indexes;
 *   every real candidate in float8 order (-inf < finite < +inf < NaN: a distance that overflowed is a row like any
 *   other), ties by lower candidate position, comes before any padding; -1 entries of cand take no part in the order
 *   and only pad: once a query's real candidates are used up the rest of its row is +inf / -1.
 * The values come from the exact vector-ALU kernel that serves pgv_hnsw_score (no matrix-core expansion).  A candidate
 * of -1 contributes no value whatever the rows hold (and with n == 0 no row is read at all).  A candidate >= n or < -1 is
 * PGV_ERR_ARG when cand is host memory; when cand is device memory it is NOT checked and the behaviour is undefined.
 * For cosine the caller passes normalised rows with PGV_NEG_IP, as elsewhere in this ABI.
 */
int			pgv_rerank(pgv_ctx * ctx, pgv_metric metric, pgv_dtype dtype, int dim, const void *queries, int nq,
					   const void *rows, int64_t n, const int64_t *cand, int kc, int k, float *out_dist, int64_t *out_idx);

/* ------------------------------------------------ sparsevec: exact distances */

/*
 * Sparse vectors travel as CSR, which is what a SparseVector datum stores (src/sparsevec.h:22-47: sorted 0-based int32
 * indices, then float values), vector after vector:
 *   ptr [n + 1]    int64_t, ptr[0] = 0, monotone; vector v owns elements ptr[v] .. ptr[v + 1] - 1
 *   idx [ptr[n]]   int32_t, strictly ascending inside a vector, 0 <= idx < dim
 *   val [ptr[n]]   float, finite
 * 1 <= dim <= 1 000 000 000 (SPARSEVEC_MAX_DIM) and at most 16 000 stored elements per vector (SPARSEVEC_MAX_NNZ), else
 * PGV_ERR_DIMS.  A vector with no stored element is legal ('{}/2'), and so is a stored 0.0.  Every array may be host or
 * device memory.  HOST arrays are validated before any launch (a ptr that is not monotone, an index out of range or
 * not ascending, a value that is not finite: PGV_ERR_ARG; too many stored elements: PGV_ERR_DIMS; the text names the
 * vector and the position); DEVICE arrays are NOT checked and the behaviour is undefined (pgv_rerank's rule for cand).
 * Host idx / val under a DEVICE row_ptr count as unchecked too: their vectors' bounds are not on the host.  (A device
 * q_ptr is copied to the host, where the queries' tiles are planned, and checked there.)
 *
 * Every value is an fp32 sum of exactly the terms the reference adds, each computed as the reference computes it;
 * only the order of the additions differs from its index order (no |a|^2 + |b|^2 - 2ab expansion): a vector's L2 /
 * L1 distance to itself is exactly 0, integer-valued data gives the reference's bits, and a sum that overflows with
 * terms of one sign is +-inf like the reference's.
 *
 * An HNSW index over sparsevec is walked through pgv_hnsw_upload_sparse / pgv_hnsw_search_sparse (the HNSW side, below),
 * with these values as its distances.  Not served: a device-side sparsevec_l2_normalize (it drops the elements that
 * round to zero and so changes the CSR: the caller normalises for cosine), the ext/ glue.  bench.py does not measure
 * these entries; tools/bench_sparse_topk.py does.
 */

/*
 * One sparse query (q_nnz stored elements at q_idx / q_val) against n sparse rows: one fmgr call per heap row in the
 * reference.  out [n] = kernel value:
 *   PGV_L2SQ    SparsevecL2SquaredDistance (src/sparsevec.c:826-869); the sqrt stays the caller's float8 post-op
 *   PGV_NEG_IP  -SparsevecInnerProduct (src/sparsevec.c:905-936, :958-966)
 *   PGV_L1      the loop of sparsevec_l1_distance (src/sparsevec.c:1018-1060)
 */
int			pgv_sparse_distance_batch(pgv_ctx * ctx, pgv_metric metric, int dim,
									  int q_nnz, const int32_t *q_idx, const float *q_val,
									  const int64_t *row_ptr, const int32_t *row_idx, const float *row_val, int64_t n,
									  float *out);

/*
 * sparsevec_cosine_distance (src/sparsevec.c:972-1011): the inner product and the two squared norms as three fp32
 * sums, `(double) ip / sqrt((double) na * (double) nb)`, clamped to [-1, 1], 1 - similarity.  An empty or all-zero
 * vector gives NaN like the reference (test/expected/sparsevec.out, cosine_distance('{}/1', '{}/1')).  out [n] float8,
 * like pgv_cosine_distance_batch.
 */
int			pgv_sparse_cosine_distance_batch(pgv_ctx * ctx, int dim,
											 int q_nnz, const int32_t *q_idx, const float *q_val,
											 const int64_t *row_ptr, const int32_t *row_idx, const float *row_val, int64_t n,
											 double *out);

/*
 * `ORDER BY emb <op> $1 LIMIT k` over a sparsevec column without an index, for a BATCH of queries: one
 * sparsevec_l2_distance / sparsevec_negative_inner_product / sparsevec_l1_distance call per heap row (the merge loops
 * of src/sparsevec.c:826-869, :905-936, :1018-1060) feeding the executor's top-N sort.  nq queries (q_ptr [nq + 1],
 * q_idx, q_val) against the same n rows: out_dist [nq x k] ascending kernel values (pgv_sparse_distance_batch's, bit for
 * bit: the same kernel), out_idx [nq x k] row indexes, ties by lower index (pgv_exact_topk's rule); entries beyond n are
 * +inf / -1.  1 <= k <= 4096, n <= 2^32.  The queries are served in chunks of min(nq, max(1, 2^30 / n)), so that a
 * chunk's distance matrix stays at or under 2^30 floats (the environment variable PGV_SPARSE_MATRIX_FLOATS, read at
 * every call, replaces the 2^30: tests reach the split with it).  For cosine the caller passes normalised vectors with
 * PGV_NEG_IP, as elsewhere in this ABI.
 */
int			pgv_sparse_topk(pgv_ctx * ctx, pgv_metric metric, int dim,
							const int64_t *q_ptr, const int32_t *q_idx, const float *q_val, int nq,
							const int64_t *row_ptr, const int32_t *row_idx, const float *row_val, int64_t n,
							int k, float *out_dist, int64_t *out_idx);

/* ----------------------------------- IVFFlat over bit strings (bit_hamming_ops) */

/*
 * Device mirror of `USING ivfflat (col bit_hamming_ops)` (sql/vector.sql:894-899, ivfflat_bit_support and its type info
 * in src/ivfutils.c:295-299, 325-339, 363-370, 411-424): centers [nlists x bytes], rows [n x bytes], bytes =
 * (nbits + 7) / 8, VARBITS payloads exactly as pgv_bit_topk / pgv_hnsw_upload_bits take them (first bit = top bit of
 * byte 0, pad bits zero, bytes counted whole); list_offsets / tids as pgv_index_upload.  1 <= nbits <= 64 000
 * (IVFFLAT_MAX_DIM * 32, src/ivfutils.c:416) else PGV_ERR_DIMS; 1 <= nlists <= 32768.
 *
 * On a bit index these entries work, with queries given as [nq x bytes] bit strings and Hamming distances returned as
 * floats (exact: at most 64 000): pgv_index_free, pgv_index_share, pgv_index_tids, pgv_index_rows, pgv_index_lists,
 * pgv_rank_lists, pgv_scan_lists, pgv_search_batch, pgv_scan_batch.
 *   pgv_rank_lists   GetScanLists (src/ivfscan.c:47-118): ascending by (distance, list id).  The SET at the boundary is
 *                    the reference's (its strict `<` at :92 admits no later list at an equal distance); the ORDER among
 *                    equal distances, which its pairing heap leaves open, is this library's rule.
 *   scan heads       ascending by (distance, insertion position); the position counts through the query's lists in
 *                    probe order and in row order inside a list.  Padding is +inf / -1.
 *   pgv_scan_lists   a NULL query gives all zeros (ZeroDistance, src/ivfscan.c:192-196).
 * These return PGV_ERR_ARG on a bit index before any launch: pgv_index_set_overlap, pgv_index_export, pgv_index_drain,
 * pgv_index_shadow_cast, pgv_query_begin, pgv_search_batch_sharded (the import wire has no field for nbits; the
 * single-query path and the lanes are float kernels).  pgv_builder_* takes a pgv_dtype and cannot be handed bits: a bit
 * index is built from pgv_bit_kmeans and pgv_bit_assign plus a stable sort by list on the caller's side.
 */
int			pgv_index_upload_bits(pgv_ctx * ctx, int nbits, int nlists, const void *centers, const int64_t *list_offsets,
								  const void *rows, const uint64_t *tids, pgv_index * *out);
int			pgv_index_nbits(const pgv_index * index);	/* 0 on a vector / halfvec index, -1 on NULL */

/*
 * AddTupleToSort's argmin (src/ivfbuild.c:183-192) under hamming_distance: the first strictly-smallest center wins.
 * centers [k x bytes], rows [n x bytes]; out_list [n], out_dist [n] (or NULL) the distance to it.  Host or device.
 */
int			pgv_bit_assign(pgv_ctx * ctx, int nbits, const void *centers, int k, const void *rows, int64_t n,
						   int32_t *out_list, float *out_dist);

/*
 * IvfflatKmeans (src/ivfkmeans.c:553-570) for the bit type info.  The reference runs Elkan (:246-485); under Hamming
 * every bound is an exact small integer or half-integer in fp32 and Hamming is a metric, so its pruning never changes
 * an outcome and it is exactly this loop: k-means++ (InitCenters, :23-91, weight = min(weight, (float) d^2), sum and
 * pick in double); iteration 0 assigns every sample to the first strictly-nearest center (:323-344); every later
 * iteration keeps a sample where it is unless a center is STRICTLY closer (:440), then takes the lowest-indexed center
 * among the strictly closest; new centers after each assignment (ComputeNewCenters + BitUpdateCenter, :205-231 and
 * src/ivfutils.c:325-339: bit = (float) sum / (float) count > 0.5, an empty cluster takes nbits RandomDouble() draws,
 * bit = (float) draw > 0.5, clusters in center order and bits in bit order); the loop stops when an iteration other
 * than the first moves nothing (:482-483).  out_iters counts like pgv_kmeans.  n == 0 is RandomCenters (:110-133):
 * every cluster is drawn.  More lists than distinct samples is no error.  n < 2^24, else PGV_ERR_ARG (the reference
 * sums +1.0f into a float, which stops counting there; below it the integer counts here are the same numbers).
 * samples [n x bytes], out_centers [k x bytes], out_closest [n] (or NULL).  max_iterations <= 0: 500.
 */
int			pgv_bit_kmeans(pgv_ctx * ctx, int nbits, const void *samples, int n, int k, int max_iterations,
						   const pgv_rng * rng, void *out_centers, int32_t *out_closest, int *out_iters);

/*
 * One iteration of it, for tests and for callers that drive the loop: io_closest[j] = -1 means "not assigned yet" (plain
 * first-strict-minimum), >= 0 the center the sample stays with unless one is strictly closer.  out_centers [k x bytes]
 * the centers after the update, out_counts [k] the cluster sizes, *out_changes the samples whose center changed.
 */
int			pgv_bit_lloyd_step(pgv_ctx * ctx, int nbits, const void *samples, int n, const void *centers, int k,
							   int32_t *io_closest, const pgv_rng * rng, void *out_centers, int32_t *out_counts,
							   int64_t *out_changes);

/* --------------------------------------------------------------- HNSW side */

/*
 * Device mirror of an HNSW index's element vectors (the `Vector data` at byte
 * 72 of every HnswElementTupleData, src/hnsw.h:372-382), addressed by a dense
 * element slot the host keeps per (blkno, offno).
 */
int			pgv_hnsw_upload(pgv_ctx * ctx, pgv_metric metric, pgv_dtype dtype, int dim,
							const void *elements, int64_t n, pgv_hnsw * *out);
void		pgv_hnsw_free(pgv_hnsw * h);
/*
 * The same with a PAYLOAD per element (0..4096 bytes in whole words) kept next to the vectors: what a scan needs to
 * turn a result element into heap TIDs (HnswElementTuple's heaptids[HNSW_HEAPTIDS] and their count,
 * src/hnsw.h:142-153, hnswgettuple src/hnswscan.c:293-311).  It rides in the elements' allocation, so an importing
 * process (pgv_hnsw_import) sees it without a table of its own; pgv_hnsw_get_payload brings the payload rows of a
 * scan's result elements to the host (element slots < 0 give zero bytes).
 */
int			pgv_hnsw_upload_payload(pgv_ctx * ctx, pgv_metric metric, pgv_dtype dtype, int dim, const void *elements,
									int64_t n, const void *payload, int payload_bytes, pgv_hnsw * *out);
int			pgv_hnsw_get_payload(pgv_hnsw * h, const int64_t *elements, int n, void *out);

/*
 * The mirror of an HNSW index over BIT strings -- `USING hnsw ((binary_quantize(embedding)::bit(n)) bit_hamming_ops)`,
 * the index the reference's README puts under the two-stage binary-quantization query (opclass sql/vector.sql:901-905,
 * FUNCTION 1 hamming_distance; type info hnsw_bit_support, src/hnswutils.c:1403-1416).  It replaces what hnswgettuple's
 * first batch (GetScanItems, src/hnswscan.c:25-56) does on such an index: the same walk, every candidate scored with
 * hamming_distance (src/bitvec.c:45-56 over BitHammingDistanceDefault, src/bitutils.c:49-73).
 *   elements [n x (nbits + 7) / 8] bytes, host or device: VARBITS payloads as pgv_bit_topk takes them, contiguous,
 *   first bit = most significant bit of byte 0, the caller's pad bits zero (bytes are counted whole, like the reference);
 *   1 <= nbits <= 64 000 (HNSW_MAX_DIM * 32), else PGV_ERR_DIMS; payload / payload_bytes as pgv_hnsw_upload_payload
 *   (NULL / 0: none).
 * metric must be PGV_BIT_HAMMING.  PGV_BIT_JACCARD is PGV_ERR_ARG here, and the text names pgv_hnsw_upload_jaccard below:
 * jaccard_distance is a float8 ratio, fp32 keys would merge distinct distances, and the reference's stop test is strict
 * on the float8 value -- so a Jaccard mirror ranks by a 32-bit INTEGER key and has an entry of its own.
 * On such a mirror pgv_hnsw_search / pgv_hnsw_score take queries [nq x (nbits + 7) / 8] in the same layout and return
 * the Hamming distances as floats (exact: at most 64 000); pgv_hnsw_score_pairs likewise; pgv_hnsw_set_graph,
 * pgv_hnsw_update_graph, pgv_hnsw_get_payload, pgv_hnsw_share and pgv_hnsw_export / pgv_hnsw_import work as on any
 * mirror (views and importers know the element type and nbits).  Every build-side entry (pgv_hnsw_build_*,
 * pgv_hnsw_link_*, pgv_hnsw_score_groups) returns PGV_ERR_ARG before any launch on a mirror of THIS entry: a bit graph is
 * built on a mirror of pgv_hnsw_upload_bits_buildable below.
 */
int			pgv_hnsw_upload_bits(pgv_ctx * ctx, pgv_bit_metric metric, int nbits, const void *elements, int64_t n,
								 const void *payload, int payload_bytes, pgv_hnsw * *out);

/*
 * The mirror of `USING hnsw (col bit_jaccard_ops)` (opclass sql/vector.sql:907-911, FUNCTION 1 jaccard_distance; the same
 * type info hnsw_bit_support): the walk of pgv_hnsw_upload_bits with every candidate scored by jaccard_distance
 * (src/bitvec.c:60-70 over BitJaccardDistanceDefault, src/bitutils.c:99-131).  Layout, limits and errors are
 * pgv_hnsw_upload_bits': elements [n x (nbits + 7) / 8] bytes, 1 <= nbits <= 64 000 else PGV_ERR_DIMS, payload the same.
 *
 * The key.  With x = popcount(a ^ b) and u = popcount(a | b) the reference's value is 1 when u - x = 0 and
 * 1 - (double) (u - x) / (double) u otherwise: the rational x / u pushed through two monotone roundings.  Two different
 * rationals with denominators <= 64 000 differ by at least 1 / 64 000^2 ~ 2.4e-10, far above a double's spacing near 1,
 * so the doubles order exactly like the rationals and equal rationals give equal doubles.  The walk ranks by
 * floor(x * S / u) in 64-bit integer arithmetic, S = 0xFFFFFF00: since 64 000^2 = 4 096 000 000 < S, two different
 * rationals are more than 1 apart after scaling, and the key is strictly monotone and injective on them.  u = 0 (two
 * empty strings) and x = u (no common bit) are distance 1: key S.  No key is 0xffffffff.  An fp32 key would merge
 * neighbouring ratios (x / u near 1 / 2 with u near 64 000 are 2.4e-10 apart, fp32 resolves 3e-8 there).
 * Ties: equal rationals -- (x, u) and (g x, g u) -- are equal keys, as they are equal float8 values in the reference, and
 * are ordered as on every other mirror (the walk's tie list; pgv_hnsw_search's note on equal distances).
 *
 * Distances handed back (pgv_hnsw_search, the scan entries and their drain, pgv_hnsw_score, pgv_hnsw_score_pairs) are
 * the (float) of the reference's float8 for the pair, bit for bit, 1.0 for no common bit included: a key does not carry
 * (x, u), so a launch scores its at most ef result elements once more and divides in IEEE double.
 *
 * On such a mirror pgv_hnsw_search, pgv_hnsw_score, pgv_hnsw_score_pairs, pgv_hnsw_set_graph, pgv_hnsw_update_graph,
 * pgv_hnsw_get_payload, pgv_hnsw_share, pgv_hnsw_export / pgv_hnsw_import (the handle carries the bit metric: an
 * importer walks with the exporter's keys) and pgv_hnsw_scan_begin / _next / _drain / _end work as on a Hamming mirror.
 * Every build-side entry returns PGV_ERR_ARG before any launch, as on a mirror of pgv_hnsw_upload_bits: a Jaccard graph
 * is built on a mirror of pgv_hnsw_upload_bits_buildable below (or comes from the reference's build).
 * Not served: ext/, which keeps handing the bit
 * opclasses to the CPU path; an IVFFlat index (the reference has no ivfflat Jaccard opclass).  bench.py does not measure
 * this entry, tools/bench_jaccard_hnsw.py does.
 */
int			pgv_hnsw_upload_jaccard(pgv_ctx * ctx, int nbits, const void *elements, int64_t n, const void *payload,
									int payload_bytes, pgv_hnsw * *out);

/*
 * A bit mirror to BUILD on: `CREATE INDEX ... USING hnsw (... bit_hamming_ops | bit_jaccard_ops)`.  metric is
 * PGV_BIT_HAMMING or PGV_BIT_JACCARD; layout, limits and errors are pgv_hnsw_upload_bits'.  The mirror behaves in every
 * entry the two mirrors above serve exactly as they do (search, score, score_pairs, scan_*, set / update_graph, payload,
 * share, export), and IN ADDITION pgv_hnsw_build_search, _build_neighbors, _build_search_keep, _build_select_kept,
 * pgv_hnsw_link_begin / _prepare / _apply / _end and pgv_hnsw_score_groups serve it with the semantics they have on a
 * dense mirror.  Distances they return and compare are floats, as HnswCandidate.distance is (the casts at
 * src/hnswutils.c:1052 and :1336): Hamming counts, or the (float) of jaccard_distance's float8 as pgv_hnsw_score_pairs
 * returns it.  Under Jaccard the SEARCH still ranks by the integer key, so every candidate list W is in the float8's order;
 * its distances are then formed from (x, u) once more.  Distinct float8 values may round to one float: the list keeps W's
 * order (the reference does not sort a new element's list again, :1351), and selection and HnswUpdateConnection compare
 * the floats, `<=` at :1052 included.
 * A view (pgv_hnsw_share) inherits the property: the host build runs on views.  An importer of its export does NOT: the
 * handle's wire format has no field for it and importers do not build -- there the build-side entries are PGV_ERR_ARG
 * as on any bit mirror.  A sparse mirror is built on through pgv_hnsw_upload_sparse_buildable, below.
 * pgv_hnsw_buildable_bits: nbits of a mirror (or view) uploaded here, 0 for every other mirror and for NULL.
 * pgv_host_hnsw_build_bits (pgv_host.h) is the build; tools/bench_bit_hnsw_build.py measures it.
 */
int			pgv_hnsw_upload_bits_buildable(pgv_ctx * ctx, pgv_bit_metric metric, int nbits, const void *elements, int64_t n,
										   const void *payload, int payload_bytes, pgv_hnsw * *out);
int			pgv_hnsw_buildable_bits(const pgv_hnsw * h);

/*
 * ---- HNSW over sparsevec elements.
 * The mirror of `USING hnsw (col sparsevec_l2_ops | sparsevec_ip_ops | sparsevec_cosine_ops | sparsevec_l1_ops)`
 * (sql/vector.sql:1189-1212; type info hnsw_sparsevec_support, src/hnswutils.c:1361-1433), the only index the reference
 * has for the type.  It replaces what hnswgettuple's first batch (GetScanItems, src/hnswscan.c:25-56) does on such an
 * index: the same walk, every candidate scored with FUNCTION 1 of the opclass -- sparsevec_l2_squared_distance,
 * sparsevec_negative_inner_product, sparsevec_l1_distance (src/sparsevec.c:826-899, :905-966, :1018-1060), each the
 * (double) of an fp32 sum, so the walk's fp32 keys are exact images of the reference's float8 distances.
 *   row_ptr / row_idx / row_val: the n elements in CSR under the rules of the sparsevec section above (host or device
 *   memory; 1 <= dim <= 1e9); metric PGV_L2SQ, PGV_NEG_IP or PGV_L1 -- cosine is PGV_NEG_IP over vectors the caller
 *   normalised, as elsewhere; payload / payload_bytes as pgv_hnsw_upload_payload (NULL / 0: none).
 * An element with more than 1000 stored elements (HNSW_MAX_NNZ, src/hnsw.h:34; HnswCheckValue's sparsevec check,
 * src/hnswutils.c:1361-1372) is PGV_ERR_DIMS; the text carries the reference's message and names the element.  Host
 * arrays are validated before any launch; a device row_ptr is copied to the host and checked there (monotone, the
 * limit); device row_idx / row_val are used unchecked (pgv_rerank's rule).  The mirror keeps index and value of a
 * stored element side by side, 8 bytes: a row the walk gathers is one contiguous run.
 *
 * On such a mirror pgv_hnsw_free, pgv_hnsw_set_graph, pgv_hnsw_update_graph, pgv_hnsw_get_payload, pgv_hnsw_device and
 * pgv_hnsw_share (a view has its own stream, scratch and visited bitmaps; the element CSR stays the owner's) work as on
 * any mirror, and pgv_hnsw_score_pairs scores element a[i] against element b[i] (b as the query).  These return
 * PGV_ERR_ARG before any launch: pgv_hnsw_search and pgv_hnsw_score (they take dense queries: use the _sparse twins),
 * pgv_hnsw_export (the handle has no fields for a second allocation; nothing can be imported), pgv_hnsw_scan_begin (it
 * takes dense query rows: an iterative scan of a sparse mirror begins with pgv_hnsw_scan_begin_sparse), and on a mirror
 * of THIS entry every pgv_hnsw_build_* and pgv_hnsw_link_* entry and pgv_hnsw_score_groups (a sparse graph is built on a
 * mirror of pgv_hnsw_upload_sparse_buildable below).  The _sparse entries on any other mirror are PGV_ERR_ARG too.
 * Not served: a device-side sparsevec_l2_normalize, the ext/ glue (ext/ returns every sparsevec opclass to
 * the CPU path); bench.py does not measure these entries, tools/bench_sparse_hnsw.py does.
 */
int			pgv_hnsw_upload_sparse(pgv_ctx * ctx, pgv_metric metric, int dim,
								   const int64_t *row_ptr, const int32_t *row_idx, const float *row_val, int64_t n,
								   const void *payload, int payload_bytes, pgv_hnsw * *out);
/*
 * A sparse mirror to BUILD on: `CREATE INDEX ... USING hnsw (... sparsevec_l2_ops | _ip_ops | _cosine_ops | _l1_ops)`.
 * Arguments, layout, limits and errors are pgv_hnsw_upload_sparse's (an element of more than 1000 stored elements is
 * PGV_ERR_DIMS with the reference's message).  The mirror behaves in every entry the plain sparse mirror serves exactly
 * as that one does (search_sparse, scan_begin_sparse, score_sparse, score_pairs, set / update_graph, payload, share),
 * and IN ADDITION pgv_hnsw_build_search, _build_neighbors, _build_search_keep, _build_select_kept, pgv_hnsw_link_begin /
 * _prepare / _apply / _end and pgv_hnsw_score_groups serve it with the semantics they have on a dense mirror.  Iterative
 * scans (pgv_hnsw_scan_begin_sparse) work as on the plain sparse mirror; export stays refused.  A view (pgv_hnsw_share)
 * inherits the property: the host build runs on views.
 *
 * WHICH SIDE IS THE QUERY.  A pair's value is an fp32 sum whose order of additions depends on which vector is the row
 * and which the query (the row's terms first, then the query's unmatched ones), so on float data swapping the two can
 * change the last bit -- dense and bit rows have no such asymmetry, and the reference's HnswGetDistance is symmetric.
 * The build compares and caches distances of one pair that reach it by different routes (a search's candidate list, the
 * pair triangles of a selection, the replays of the lists a batch links into, the host forms), so on a buildable sparse
 * mirror the BUILD-SIDE value of the pair {a, b} of element slots is always
 *     row = the element in the smaller slot, query = the element in the larger slot,
 * i.e. pgv_hnsw_score_pairs(a = min, b = max) bit for bit.  pgv_hnsw_score_groups and every triangle the build-side
 * entries score follow it (with PGV_HNSW_PAIRS_GATHER=1 too).  pgv_hnsw_score_pairs itself keeps "b is the query",
 * whatever the slots.  pgv_hnsw_build_search scores with the inserted element as the query, as every walk does; see there.
 * pgv_hnsw_buildable_sparse: dim of a mirror (or view) uploaded here, 0 for every other mirror and for NULL.
 * pgv_host_hnsw_build_sparse (pgv_host.h) is the build; tools/bench_sparse_hnsw_build.py measures it.
 */
int			pgv_hnsw_upload_sparse_buildable(pgv_ctx * ctx, pgv_metric metric, int dim,
											 const int64_t *row_ptr, const int32_t *row_idx, const float *row_val, int64_t n,
											 const void *payload, int payload_bytes, pgv_hnsw * *out);
int			pgv_hnsw_buildable_sparse(const pgv_hnsw * h);
/* the element slots of a mirror of any kind or of a view (-1: NULL): what a host build checks its rows against */
int64_t		pgv_hnsw_elements(const pgv_hnsw * h);
/*
 * pgv_hnsw_score over a sparse mirror (HnswSearchLayer's candidate scoring, src/hnswutils.c:908-934, with the sparsevec
 * FUNCTION 1): pair i scores element slot[i] against query query_of[i] (NULL: query 0) of the nq queries in CSR.  The
 * values are pgv_sparse_distance_batch's for the same two vectors, bit for bit: the same terms in the same order of
 * additions, an empty intersection's negative inner product +0.0.  Queries are not elements: a query may store up to
 * 16 000 elements (SPARSEVEC_MAX_NNZ; HnswCheckValue, src/hnswutils.c:413, is the index-value path); host query arrays
 * are validated like pgv_sparse_topk's.
 */
int			pgv_hnsw_score_sparse(pgv_hnsw * h, const int64_t *q_ptr, const int32_t *q_idx, const float *q_val, int nq,
								  const int32_t *slot, const int32_t *query_of, int64_t npairs, float *out);
/*
 * pgv_hnsw_search over a sparse mirror, word for word (GetScanItems, src/hnswscan.c:25-56; HnswSearchLayer,
 * src/hnswutils.c:824-987): greedy descent, layer 0 with ef_search, out_scored = so->tuples; queries in CSR as
 * pgv_hnsw_score_sparse takes them.  The query's pairs sit in LDS next to the walk's state: ef_search, m and the
 * batch's longest query together may need at most 150 KiB, else PGV_ERR_ARG before any launch (the text names the
 * three); a 16 000-element query fits with ef_search 40 and m 16.
 */
int			pgv_hnsw_search_sparse(pgv_hnsw * h, const int64_t *q_ptr, const int32_t *q_idx, const float *q_val, int nq,
								   int ef_search, int k, int64_t *out_elem, float *out_dist, int64_t *out_scored);

/*
 * The HNSW mirror across processes, like pgv_index_export / pgv_index_import: the element vectors and the graph
 * (set with pgv_hnsw_set_graph) stay in the exporting process's HBM, importers map them read-only and search on
 * their own context (stream, visited bitmaps).  Graph patches by the owner (pgv_hnsw_update_graph) are seen by the
 * importers; the entry point travels inside the handle, so a new entry point -- like a pgv_hnsw_set_graph by the owner,
 * which reallocates the graph -- needs a new export.
 */
int			pgv_hnsw_export(pgv_hnsw * h, pgv_index_handle * out);
/*
 * A view of a mirror for ANOTHER context of the same process (its own stream, scratch and visited bitmaps; the
 * element rows, the payload and the graph stay the owner's and follow the owner's pgv_hnsw_set_graph /
 * pgv_hnsw_update_graph): pgv_index_share's twin.  Searches, scoring and pgv_hnsw_update_graph work through a view
 * (the patch lands in the owner's graph); pgv_hnsw_set_graph and pgv_hnsw_export do not.  The HNSW build runs the next
 * batch's searches and the graph patches on views while the current batch's lists are replayed
 * (pgvector_amd/host/hnsw_build.c).  One thread per handle at a time; free the views before the owner.
 */
int			pgv_hnsw_share(pgv_hnsw * h, pgv_ctx * ctx, pgv_hnsw * *out);
int			pgv_hnsw_device(const pgv_hnsw * h);	/* the device the mirror lives on (-1: NULL) */
int			pgv_hnsw_import(pgv_ctx * ctx, const pgv_index_handle * handle, pgv_hnsw * *out);

/*
 * The candidate-scoring loop of HnswSearchLayer (src/hnswutils.c:908-934,
 * HnswLoadElementImpl :533-571): distances from queries to gathered elements.
 * Pair i scores element slot[i] against query query_of[i] (query_of == NULL ->
 * all pairs use query 0).  One call serves one expansion step of many
 * concurrent searches.
 *   queries [nq x dim], slot [npairs], query_of [npairs] or NULL, out [npairs]
 */
int			pgv_hnsw_score(pgv_hnsw * h, const void *queries, int nq,
						   const int32_t *slot, const int32_t *query_of, int64_t npairs, float *out);

/*
 * The graph the scan walks, flattened: the meta page's m and entry point
 * (src/hnswutils.c:298-328) and, per element slot, its level and neighbor tuple
 * (src/hnsw.h:384-392: (level + 2) * m slots, layer lc starting at
 * (level - lc) * m, src/hnswutils.c:786; -1 = invalid TID).  Copied to the device.
 *   levels [n], nbr_start [n + 1] (offsets into nbr), nbr [nbr_start[n]]
 */
int			pgv_hnsw_set_graph(pgv_hnsw * h, int m, int32_t entry, const int32_t *levels,
							   const int64_t *nbr_start, const int32_t *nbr);

/*
 * hnswgettuple's first batch on the device (GetScanItems, src/hnswscan.c:25-56):
 * greedy descent with ef = 1 through the upper layers, then HnswSearchLayer with
 * ef_search on layer 0 (src/hnswutils.c:824-987), one workgroup per query, no host
 * round trips.  Needs pgv_hnsw_set_graph.  Queries already normalised for cosine
 * (src/hnswscan.c:92-114).
 *   queries    [nq x dim]
 *   out_elem   [nq x k] element slots nearest first, -1 padded (k <= ef_search)
 *   out_dist   [nq x k] FUNCTION 1 distances, +inf padded
 *   out_scored [nq] or NULL: so->tuples, the number of elements scored on layer 0
 */
int			pgv_hnsw_search(pgv_hnsw * h, const void *queries, int nq, int ef_search, int k,
							int64_t *out_elem, float *out_dist, int64_t *out_scored);

/* ------------------------------------------------------ HNSW iterative scans */

/*
 * hnsw.iterative_scan on the device (hnswgettuple's loop, src/hnswscan.c:242-327): a scan over a batch of queries whose
 * batches are fetched one launch at a time.  A query's first batch is GetScanItems (src/hnswscan.c:25-56) -- the walk of
 * pgv_hnsw_search, tie handling included -- and every later one is ResumeScanItems (:61-87): HnswSearchLayer on layer 0
 * (src/hnswutils.c:824-987) from the ef_search nearest of the candidates the earlier batches discarded (`discarded`,
 * :936-946, :967-973), with the visited set carried over (initVisited == false, :867-874).  The scan keeps per QUERY a
 * visited bitmap over the mirror's elements, the pool of discarded candidates and so->tuples.
 *
 * The order among equal distances is unspecified in the reference (pairing-heap internals); here the pool keeps its
 * entries in the order they were discarded (per merged batch: the entries pushed out of W, in W's order, then the batch's
 * own that did not fit, in batch order) and "nearest" is by (distance, position in the pool).  Without ties every batch
 * holds the reference's elements, distances and so->tuples.
 *
 * The caller's to do: end every scan of a mirror (or of its views) before pgv_hnsw_free of that handle; the reference's
 * memory limit (hnsw.scan_mem_multiplier x work_mem, src/hnswscan.c:153-156, :259) has no counterpart: discard_cap takes its
 * place, and a pool that would outgrow it ends the scan with PGV_ERR_NOMEM.
 */
typedef struct pgv_hnsw_scan pgv_hnsw_scan;

/*
 * hnswbeginscan / hnswrescan's part (src/hnswscan.c:130-184): stages the queries as pgv_hnsw_search takes them (fp32 / fp16
 * rows, bit strings on a bit mirror) and allocates the state; launches nothing.  Works on views (pgv_hnsw_share) and
 * imported mirrors, on that handle's context and stream.  Several scans may be open on one mirror and pgv_hnsw_search
 * may run between their batches: the scan owns its visited sets.
 *   ef_search    1..1000 (src/hnsw.c:93-94)
 *   discard_cap  pool entries per query; 0 = min(n, 65536).  State per query: 8 * discard_cap + 4 * (n / 32 + 2) + 16
 *                bytes and the query row
 * PGV_ERR_ARG: a sparse mirror (it takes sparse queries: pgv_hnsw_scan_begin_sparse), no graph set, ef_search out of
 * range.  PGV_ERR_NOMEM: the state does not fit (the text has the byte count).
 */
int			pgv_hnsw_scan_begin(pgv_hnsw * h, const void *queries, int nq, int ef_search, int64_t discard_cap,
								pgv_hnsw_scan * *out);
/*
 * pgv_hnsw_scan_begin on a sparse mirror (pgv_hnsw_upload_sparse, _buildable, or a view of either): hnswbeginscan /
 * hnswrescan for `USING hnsw (... sparsevec_*_ops)`.  The queries come in CSR and are validated and staged as
 * pgv_hnsw_search_sparse's: host arrays are checked before anything else, a device q_ptr is copied to the host and checked,
 * a query may store up to 16 000 elements.  The scan keeps ITS OWN device copy of the queries for its lifetime -- the
 * offsets, the indices and the values as three arrays, the layout the walk stages a query from (a stored element takes
 * 8 bytes, as it would side by side) -- so the caller may reuse its arrays as soon as the call returns, and
 * pgv_hnsw_search_sparse may run between the scan's batches.  Launches nothing.
 *   ef_search, discard_cap  as pgv_hnsw_scan_begin.  State per query: 8 * discard_cap + 4 * (n / 32 + 2) + 16 bytes, and
 *                           8 bytes per offset + 8 bytes per stored element of the query copy
 * pgv_hnsw_scan_next, _drain and _end serve the scan as they serve any other; the order among equal distances is the one
 * described above ((distance, position in the pool)), and without ties every batch holds the reference's elements,
 * distances and so->tuples.  A batch's first is pgv_hnsw_search_sparse(ef_search, k = ef_search), bit for bit.
 * The query's pairs sit in LDS next to the walk's state and the entry step's: ef_search, m and the SCAN's longest query
 * (whichever queries a batch wants) together may need at most 150 KiB, checked HERE (the text names the three).
 * PGV_ERR_ARG: not a sparse mirror, no graph set, ef_search outside 1..1000, a negative discard_cap, a NULL handle / out /
 * q_ptr, a query array that breaks the sparsevec rules, the LDS need.  PGV_ERR_NOMEM: the state does not fit (the text
 * has the byte count).  *out is NULL after every error.
 */
int			pgv_hnsw_scan_begin_sparse(pgv_hnsw * h, const int64_t *q_ptr, const int32_t *q_idx, const float *q_val, int nq,
									   int ef_search, int64_t discard_cap, pgv_hnsw_scan * *out);
/*
 * The next batch of every query with want[q] != 0 (want == NULL: all of them), one launch, one workgroup per query:
 * GetScanItems for a query's first batch, ResumeScanItems (src/hnswscan.c:61-87) afterwards.  The graph is read as it
 * stands at the call: a pgv_hnsw_update_graph between two batches is seen by the later one (the reference takes its
 * lock per batch as well, src/hnswscan.c:278-282).
 *   want        [nq] bytes or NULL
 *   out_elem    [nq x ef_search] element slots nearest first, -1 padded
 *   out_dist    [nq x ef_search] FUNCTION 1 distances, +inf padded
 *   out_count   [nq] entries of the batch; 0: the query is exhausted, was not wanted, or the index is empty
 *   out_scored  [nq] or NULL: so->tuples so far
 *   out_left    [nq] or NULL: candidates left in the pool
 * PGV_ERR_NOMEM when a query's pool would overflow (never written past; the text names the query and the capacity);
 * every later call on the scan returns the same error.  The mirror is unaffected.
 */
int			pgv_hnsw_scan_next(pgv_hnsw_scan * s, const uint8_t *want, int64_t *out_elem, float *out_dist,
							   int32_t *out_count, int64_t *out_scored, int64_t *out_left);
/*
 * The hnsw.max_scan_tuples branch of hnswgettuple (src/hnswscan.c:259-266: past the limit the discarded candidates are
 * returned nearest first, the graph is not walked any more), in bulk: removes and returns the `count` (1..1000) nearest
 * remaining pool entries of every wanted query, by (distance, position).
 *   out_elem / out_dist [nq x count], out_count [nq]
 */
int			pgv_hnsw_scan_drain(pgv_hnsw_scan * s, const uint8_t *want, int count, int64_t *out_elem, float *out_dist,
								int32_t *out_count);
/*
 * hnswgettuple's loop under a filter (src/hnswscan.c:242-327: hnsw.iterative_scan with a WHERE clause) for every query with
 * want[q] != 0 (NULL: all), in ONE launch: the workgroup that takes a query keeps it, batch after batch, until it has its k
 * rows, its pool is empty, or -- past max_scan_tuples -- the pool has been drained.  Per query:
 *     emitted = 0; prev = the lowest key
 *     while emitted < k:
 *         batch = the pool's ef_search nearest (pgv_hnsw_scan_drain) if the scan has started and so->tuples >= max_scan_tuples,
 *                 else the next batch (pgv_hnsw_scan_next)
 *         if the batch is empty: stop
 *         for every (element, key) of the batch, nearest first, while emitted < k:
 *             strict: an element with key < prev is dropped; otherwise prev = key
 *             if the element's keep bit is set (or keep is NULL): emit (element, distance)
 * Works on any scan -- dense, bit (Hamming or Jaccard) and sparse mirrors, views and imported mirrors --, fresh or with
 * batches already taken.
 *   want         [nq] bytes or NULL
 *   keep         a bitmap over element slots, host or device: element e is bit e & 31 of word e >> 5.  NULL keeps every
 *                element.  keep_stride == 0: one bitmap of (n + 31) / 32 words for every query; otherwise query q's
 *                begins at keep + q * keep_stride, keep_stride >= (n + 31) / 32
 *   k            1..4096 rows per query
 *   max_scan_tuples  >= 1 (hnsw.max_scan_tuples)
 *   strict       hnsw.iterative_scan = strict_order; it compares the walk's 32-bit keys, which order (and tie) as the
 *                reference's float8 distances do -- under bit_jaccard_ops too, where two keys may share one float
 *   out_elem     [nq x k] element slots in emission order, -1 padded;  out_dist [nq x k] +inf padded: for an element the
 *                very float pgv_hnsw_scan_next hands back for it
 *   out_count    [nq] rows emitted
 *   out_scored   [nq] or NULL: so->tuples at the end;  out_batches [nq] or NULL: the walks plus drains this call took for
 *                the query;  out_left [nq] or NULL: entries left in the pool
 * Every output may be host or device memory.  An unwanted query gets count 0, padding, its current so->tuples, and its
 * state untouched.
 * Afterwards the scan's state is its state after the last batch taken: a second call, a pgv_hnsw_scan_next or a _drain
 * continues from there.  `prev` and the undelivered rest of the last batch are NOT kept: the elements behind the k-th
 * emitted row of that batch are gone, as they are for a caller that stops reading pgv_hnsw_scan_next's rows early.
 * PGV_ERR_ARG, before any launch: a NULL scan / out_elem / out_dist / out_count, k outside 1..4096, max_scan_tuples < 1, a
 * keep_stride other than 0 below the mirror's (n + 31) / 32 words.  PGV_ERR_NOMEM as pgv_hnsw_scan_next: a query whose
 * pool would overflow ends flagged, the text names it, every later call on the scan repeats the error.
 */
int			pgv_hnsw_scan_filtered(pgv_hnsw_scan * s, const uint8_t *want, const uint32_t *keep, int64_t keep_stride,
								   int k, int64_t max_scan_tuples, int strict, int64_t *out_elem, float *out_dist,
								   int32_t *out_count, int64_t *out_scored, int32_t *out_batches, int64_t *out_left);
/* hnswendscan (src/hnswscan.c:336-345): waits for the handle's stream and frees the state; before pgv_hnsw_free */
void		pgv_hnsw_scan_end(pgv_hnsw_scan * s);

/* ------------------------------------------------------ HNSW build side */

/*
 * HnswFindElementNeighbors' searches (src/hnswutils.c:1280-1357) for a batch of elements being
 * inserted: from the current entry point, greedy descent (ef = 1) through the layers above each
 * element's insert level, then HnswSearchLayer with ef_construction on every layer from
 * min(insert level, entry level) down to 0.  The elements are slots of the mirror (their vectors
 * are the queries); none of them is linked into the graph yet, so none can be found.  Returns each
 * searched layer's W -- the candidate list SelectNeighbors works on -- nearest first.
 *   elements [nq], insert_levels [nq]
 *   out_ids / out_dist [nq x layer_cap x ef_construction], out_count [nq x layer_cap] (0 = layer not searched)
 * On a buildable SPARSE mirror the search scores with the inserted element as the query, as every walk does:
 * out_dist = pgv_hnsw_score_pairs(candidate, element).  pgv_host_hnsw_build_sparse inserts in slot order and a batch does
 * not see itself, so every candidate sits in a smaller slot than the element and these are the build-side values of the
 * orientation rule (pgv_hnsw_upload_sparse_buildable: the smaller slot is the row).  A direct caller who inserts out of
 * slot order gets (row = candidate, query = element) all the same, which for a candidate in a LARGER slot may differ in
 * the last bit from what pgv_hnsw_score_groups gives the pair.
 */
int			pgv_hnsw_build_search(pgv_hnsw * h, const int32_t *elements, const int32_t *insert_levels, int nq,
								  int ef_construction, int layer_cap,
								  int32_t *out_ids, float *out_dist, int32_t *out_count);

/*
 * HnswFindElementNeighbors whole (src/hnswutils.c:1280-1357) for a batch of elements being inserted: the searches of
 * pgv_hnsw_build_search, then SelectNeighbors (:1064-1165; CheckElementCloser :1040-1059) over every searched layer's
 * candidate list ON THE DEVICE -- the candidate lists and their pair distances never leave it.  A new element's list has
 * no cached closer flags, so the selection is the plain sweep: nearest candidate first, closer(e) = no neighbor chosen so
 * far is at distance <= d(e, element) from e; chosen while fewer than lm (2m on layer 0, m above), then the rejected ones
 * fill up to lm, nearest first (:1146-1148); a list of at most lm candidates is taken whole in W's furthest-first order.
 *   elements [nq], insert_levels [nq]
 *   out_ids / out_dist / out_closer [nq x layer_cap x 2m]: the neighbors in the order the reference's r holds them (what
 *       AddConnections stores, :1243-1251), their distances, their `closer` flags; out_count [nq x layer_cap]
 *   out_pairs (or NULL): pair distances computed (profiling)
 */
int			pgv_hnsw_build_neighbors(pgv_hnsw * h, const int32_t *elements, const int32_t *insert_levels, int nq,
									 int ef_construction, int layer_cap,
									 int32_t *out_ids, float *out_dist, uint8_t *out_closer, int32_t *out_count,
									 int64_t *out_pairs);

/*
 * pgv_hnsw_build_neighbors in two halves, for a build that overlaps them (between pgv_hnsw_link_begin and _end): the
 * searches of a batch, whose candidate lists are kept on the device in slot 0 or 1 of the mirror's build state -- when it
 * returns the searches are over and the tuples may be rewritten --, and SelectNeighbors over a kept slot, from any view
 * of the mirror on that view's stream (outputs as pgv_hnsw_build_neighbors).  The searches of batch n + 2 (one view, the
 * other slot) then run beside the selection of batch n + 1 (another view).
 */
int			pgv_hnsw_build_search_keep(pgv_hnsw * h, const int32_t *elements, const int32_t *insert_levels, int nq,
									   int ef_construction, int layer_cap, int slot);
int			pgv_hnsw_build_select_kept(pgv_hnsw * h, int slot, int32_t *out_ids, float *out_dist, uint8_t *out_closer,
									   int32_t *out_count, int64_t *out_pairs);

/*
 * The graph updates of the in-memory build on the device: HnswUpdateNeighborsInMemory -> HnswUpdateConnection
 * (src/hnswbuild.c:376-405, src/hnswutils.c:1183-1231) for a batch of new elements at once -- every neighbor list they
 * chose replayed by one GPU lane with the reference's SelectNeighbors (sorted candidates, cached closer flags, pruned
 * connections kept, the dropped neighbor's place handed to the newcomer), the pair distances CheckElementCloser looks up
 * scored on the device next to it.  Between _begin and _end the mirror carries, per neighbor-tuple slot, the neighbor's
 * distance and closer flag; the tuples themselves (what the searches read) are rewritten in place.
 *
 *   pgv_hnsw_link_begin    after pgv_hnsw_set_graph with every tuple empty (-1): allocates the state
 *   pgv_hnsw_link_prepare  the batch: elements [nq], linked [nq] (0: a duplicate, left out) and their neighbor lists as
 *                          pgv_hnsw_build_neighbors returned them ([nq x layer_cap x 2m] + counts).  Every (new element,
 *                          chosen neighbor, layer) is a link request; they are grouped by neighbor list on the device,
 *                          the newcomers of a list in heap order (as the reference's loop would meet them).  Scores
 *                          every pair the lists' selections can look up -- a list without cached flags: all of them;
 *                          otherwise those that involve a newcomer -- and returns while that runs
 *   pgv_hnsw_link_apply    replays the lists, then puts the batch's own elements in place; sets the entry point.  The
 *                          caller keeps searches that read the old tuples away (they have returned); later searches on
 *                          any stream see the new ones
 *                          Nothing in it waits for the device: it returns with everything enqueued, and a search posted
 *                          right behind it (another view) starts on the device when the last kernel is through
 *   pgv_hnsw_link_end      out_nbr [total slots] (or NULL): the finished tuples; out_pairs / out_deferred (or NULL): the
 *                          member-member pair distances scored for, and the number of, lists whose replay needed the
 *                          second round, over the whole build; frees the state
 * pgv_hnsw_link_prepare's out_pairs (or NULL): pair distances scored for the batch's first round.
 */
int			pgv_hnsw_link_begin(pgv_hnsw * h);
int			pgv_hnsw_link_prepare(pgv_hnsw * h, const int32_t *elements, const uint8_t *linked, int nq, int layer_cap,
								  const int32_t *sel_ids, const float *sel_dist, const uint8_t *sel_closer,
								  const int32_t *sel_count, int64_t *out_pairs);
int			pgv_hnsw_link_apply(pgv_hnsw * h, int32_t entry);
int			pgv_hnsw_link_end(pgv_hnsw * h, int32_t *out_nbr, int64_t *out_pairs, int64_t *out_deferred);

/*
 * Distances between pairs of elements of the mirror, out[i] = d(a[i], b[i]): CheckElementCloser's
 * HnswGetDistance between a candidate and an already selected neighbor (src/hnswutils.c:1040-1059),
 * batched over every pair a batch of inserts can need.
 */
int			pgv_hnsw_score_pairs(pgv_hnsw * h, const int32_t *a, const int32_t *b, int64_t npairs, float *out);
/*
 * The same distances for pairs given as GROUPS (the lists a batch of inserts touches): group g holds the
 * element slots ids[ids_start[g] .. ids_start[g + 1]) = its locals 0 .. n-1 and asks for the pairs (u, v), v < u,
 * of the locals u >= from[g], u ascending then v ascending (from = 1: the whole triangle; from = the number of old
 * members: only the pairs that involve a newcomer).  The pairs are expanded on the device, so a list of n slots
 * crosses the bus instead of up to n (n - 1) / 2 pairs of them.
 *   ids [ids_start[ngroups]], ids_start [ngroups + 1], from [ngroups], pair_start [ngroups + 1] (all host or device)
 *   out [pair_start[ngroups]]: group g's distances start at pair_start[g]
 */
int			pgv_hnsw_score_groups(pgv_hnsw * h, const int32_t *ids, const int64_t *ids_start, const int32_t *from,
								  const int64_t *pair_start, int ngroups, int64_t nids, int64_t npairs, float *out);


/*
 * The graph after a batch of inserts: new entry point and the rewritten neighbor tuples
 * (HnswUpdateNeighborsInMemory / AddConnections, src/hnswbuild.c:376-431).  Element elements[i]'s
 * whole tuple is tuples[tuple_offsets[i] .. tuple_offsets[i + 1]) in the layout of pgv_hnsw_set_graph;
 * tuple_offsets is host memory.  Ordered on the device with later searches through the mirror AND through its views
 * (pgv_hnsw_share), whichever of them ran the patch; searches that still read the old tuples must have returned before
 * the call (every search call ends synchronized), and patches of one mirror are issued one at a time (the caller's
 * business when several threads hold views: pgv_host_hnsw_build gives them all to one helper thread).
 */
int			pgv_hnsw_update_graph(pgv_hnsw * h, int32_t entry, const int32_t *elements, int nupd,
								  const int64_t *tuple_offsets, const int32_t *tuples);

/* ------------------------------------------------------ HNSW vacuum side */

/*
 * Dead elements of a mirror: bit e & 31 of word e >> 5 says that element e has heap TIDs (heaptidsLength != 0: what
 * CountElement, src/hnswutils.c:715-728, and RemoveElements, :1236-1259, look at while hnswvacuum repairs the graph,
 * src/hnswvacuum.c:379-502).  live [(n + 31) / 32] words, host or device; any other word count is PGV_ERR_ARG before any
 * launch; NULL: every element is live again (words is ignored).  The bitmap is copied to the device, kept with the
 * mirror and seen by its views (pgv_hnsw_share), whichever of them set it.  The call waits for its own handle's stream
 * and then replaces the bitmap: pgv_hnsw_repair_neighbors calls through OTHER views of the mirror must have returned
 * before it (each ends synchronized), as searches must before pgv_hnsw_update_graph.
 *
 * ONLY pgv_hnsw_repair_neighbors reads it.  pgv_hnsw_search, pgv_hnsw_scan_*, the build-side entries and every other
 * entry ignore it and behave bit for bit as on a mirror on which nothing was ever marked dead: like the reference's
 * HnswSearchLayer with skipElement == NULL they walk through dead elements, and dropping those from the answers is the
 * caller's filter (pgv_hnsw_scan_filtered's keep bitmap has this very layout).
 *
 * Dense mirrors only (pgv_hnsw_upload / pgv_hnsw_upload_payload and their views, fp32 and fp16, every metric): on a bit,
 * Jaccard, sparse or imported mirror pgv_hnsw_set_live and pgv_hnsw_repair_neighbors return PGV_ERR_ARG before any launch
 * and the text names the mirror kind.  pgv_hnsw_live_count: the bits set among the n elements (n while no bitmap is
 * set); -1 for a NULL handle and for those mirror kinds (pgv_last_error names the kind).
 */
int			pgv_hnsw_set_live(pgv_hnsw * h, const uint32_t *live, int64_t words);
int64_t		pgv_hnsw_live_count(const pgv_hnsw * h);

/*
 * HnswFindElementNeighbors(..., existing = true) (src/hnswutils.c:1280-1357), what RepairGraphElement
 * (src/hnswvacuum.c:226-274) runs for an element with a deleted neighbor, for a batch of LINKED elements of the mirror
 * against the graph as it stands:
 *   - each element's level is its own; layers above it are descended with ef = 1 (:1306-1310), every layer from
 *     min(level, entry level) down is searched with ef_construction + 1 (:1316-1317: the element finds itself);
 *   - the searches count only live elements towards ef (CountElement, :715-728, at :884 and :962): alwaysAdd = wlen < ef,
 *     otherwise an element is admitted when strictly nearer than W's furthest; a live admission raises wlen, which is
 *     never lowered, and once wlen > ef evicts W's furthest whatever it is; a dead admission evicts nothing (:908-975).
 *     W is therefore not bounded by ef;
 *   - after a layer's search W, nearest first, loses the element itself and the dead (RemoveElements, :1236-1259) and
 *     goes through SelectNeighbors on the device as in pgv_hnsw_build_neighbors (plain sweep, no cached closer flags);
 *     the next layer starts from the unstripped W (:1355).
 * W holds ef_construction + 1 + dead_cap entries in a workgroup's LDS (PGV_ERR_ARG before any launch when that does not
 * fit; the text has the byte count; pgv_hnsw_repair_dead_cap_max: the largest dead_cap that fits, -1: none).  A search
 * that would need more stops: out_status[q] = 1, every count of that element is 0, the other elements are unaffected and
 * no error is raised -- the caller redoes it with a larger dead_cap.  It is never a silently shorter list.  On a graph of
 * one layer a dead_cap of the number of dead elements cannot overflow; with more layers a dead element evicted on one
 * layer can be admitted again on the next, so the certain bound is that number times the layers searched.
 *   elements [nq] (host: checked against the mirror's slots; device: not checked, a slot outside the mirror gets counts 0)
 *   out_ids / out_dist / out_closer [nq x layer_cap x 2m], out_count [nq x layer_cap]: as pgv_hnsw_build_neighbors
 *   out_status [nq]; out_pairs (or NULL): pair distances computed
 */
int			pgv_hnsw_repair_neighbors(pgv_hnsw * h, const int32_t *elements, int nq, int ef_construction, int layer_cap,
									  int dead_cap, int32_t *out_ids, float *out_dist, uint8_t *out_closer,
									  int32_t *out_count, int32_t *out_status, int64_t *out_pairs);
int			pgv_hnsw_repair_dead_cap_max(const pgv_hnsw * h, int ef_construction);

#ifdef __cplusplus
}
#endif
#endif							/* PGV_HIP_H */
