/*
 * hnsw_repair.c -- hnswvacuum's RepairGraph (src/hnswvacuum.c:379-502) over a graph held in memory, with every search,
 * selection and pair distance on the GPU.
 *
 * The reference repairs one element at a time: RepairGraphElement (:226-274) rebuilds the element's own tuple with
 * HnswFindElementNeighbors(..., existing = true) and then runs HnswUpdateNeighborsOnDisk (src/hnswinsert.c:546-580) for
 * every neighbor it chose.  Here a BATCH of elements is repaired "at once" the way hnsw_build.c inserts a batch: all of
 * them search the graph as it stood when the batch began (one pgv_hnsw_repair_neighbors launch), then their own tuples and
 * their back links are applied in element order.  With max_batch = 1 this IS the reference's serial loop.
 *
 * Applying a batch in element order, list by list.  A neighbor list (owner, layer) is changed by two kinds of event: the
 * owner's own repair, which overwrites the whole tuple, and the back link of a batch element that chose the owner.  A back
 * link that comes BEFORE the owner's own repair in element order is overwritten by it and has no other effect, so it is
 * dropped; what is left per list is "the tuple as the batch found it, or as the owner's repair left it" followed by the
 * back links of later elements in element order -- and lists do not depend on each other.  A back link needs distances
 * only when it comes to HnswUpdateConnection (a full list without a dead member); those lists wait, the pairs of all
 * waiting lists are scored in one pgv_hnsw_score_groups call, and they go on -- as many rounds as the busiest list has
 * reselections.  The selection itself is hnsw_build.c's (pgv_host_hnsw_update_index).
 */
#include "pgv_host.h"

#include <stdlib.h>
#include <string.h>
#include <time.h>

/*
 * The vacuum-side entries of the device library are weak references: the host glue also links, whole, into programs that
 * stand in for the device with an older set of entries (tests/c/mock_hip.c); there pgv_host_hnsw_repair reports that the
 * entries are missing instead of keeping every such program from linking -- or finds the program's own stand-ins
 * (tests/c/hnsw_repair_asan_driver.c).  Once the mock has the entries the pragmas can go.
 */
#pragma weak pgv_hnsw_set_live
#pragma weak pgv_hnsw_repair_neighbors
#pragma weak pgv_hnsw_repair_dead_cap_max

extern int	pgv_host_fail(int code, const char *fmt,...);
extern int	pgv_host_hnsw_update_index(const int32_t *members, int lm, int32_t newcomer, float new_dist, const float *tri);
extern int	pgv_host_hnsw_cancelled(void);

#define DEAD_CAP_CARRY 1024

typedef struct
{
	int32_t		owner;
	int32_t		lc;
	int32_t		pos;			/* the linking element's place in the batch */
	int32_t		e;
	float		dist;			/* d(e, owner) as e's search found it */
}			backlink;

typedef struct
{
	int64_t		next,
				end;			/* its back links still to apply: events[next .. end) */
	int64_t		tri_at;			/* where the pairs of events[next] start in the reply, or -1 */
}			listrun;

typedef struct
{
	pgv_hnsw   *mirror;
	int64_t		n;
	const int32_t *levels;
	const int64_t *nbr_start;
	int32_t    *nbr;
	const uint32_t *live;
	int			m,
				efc,
				dead_cap,
				dead_cap_max;
	int32_t		entry;
	pgv_hnsw_repaired *out;
	/*
	 * Growable arrays: every one has its own capacity, NAME_cap, and is given room through ROOM() alone.
	 * A batch's selections: sel_ids / sel_dist / sel_closer [nb x lcap x 2m], sel_cnt [nb x lcap], status [nb]; the redo of
	 * overflowed elements sits behind them in the same arrays (room for 2 nb elements); redo [2 nb]: which they are
	 */
	int32_t    *sel_ids;
	float	   *sel_dist;
	uint8_t    *sel_closer;
	int32_t    *sel_cnt;
	int32_t    *status;
	int32_t    *redo;
	int64_t		sel_ids_cap,
				sel_dist_cap,
				sel_closer_cap,
				sel_cnt_cap,
				status_cap,
				redo_cap;
	int32_t    *pos_of;			/* [n] place in the current batch, or -1 */
	uint8_t    *patched;		/* [n] tuple changed in the current batch */
	int32_t    *patch_list;
	int64_t		npatched,
				patch_list_cap;
	backlink   *events;
	int64_t		nevents,
				events_cap;
	listrun    *runs;
	int64_t		nruns,
				runs_cap;
	/* one round's scoring request and its reply */
	int32_t    *g_ids;
	int64_t    *g_start;
	int32_t    *g_from;
	int64_t    *g_pair;
	int64_t		g_ids_cap,
				g_start_cap,
				g_from_cap,
				g_pair_cap;
	float	   *tri;
	int64_t		tri_cap;
	/* the patch: the changed tuples whole, tup_off [npatched + 1] where each starts in tup */
	int64_t    *tup_off;
	int32_t    *tup;
	int64_t		tup_off_cap,
				tup_cap;
}			repair;

static double
now_secs(void)
{
	struct timespec ts;

	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (double) ts.tv_sec + 1e-9 * (double) ts.tv_nsec;
}

static inline int
layer_m(int m, int lc)
{
	return lc == 0 ? 2 * m : m;
}

static inline int
is_live(const repair * R, int32_t e)
{
	return (R->live[e >> 5] >> (e & 31)) & 1u;
}

static int
grow(void **p, int64_t *cap, int64_t want, size_t item)
{
	void	   *q;
	int64_t		c = *cap;

	if (want <= c)
		return PGV_OK;
	c = c < 64 ? 64 : c;
	while (c < want)
		c *= 2;
	q = realloc(*p, (size_t) c * item);
	if (!q)
		return pgv_host_fail(PGV_ERR_NOMEM, "pgv_host_hnsw_repair: out of host memory");
	*p = q;
	*cap = c;
	return PGV_OK;
}

/* room for `want` items in R->name, whose capacity is R->name_cap: the one way these arrays are sized */
#define ROOM(R, name, want) grow((void **) &(R)->name, &(R)->name##_cap, (want), sizeof(*(R)->name))

/* NeedsUpdated (src/hnswvacuum.c:179-220): a neighbor being deleted, or the last slot of layer 0 empty */
static int
needs_updated(const repair * R, int32_t e)
{
	const int64_t a = R->nbr_start[e],
				b = R->nbr_start[e + 1];

	for (int64_t i = a; i < b; i++)
		if (R->nbr[i] >= 0 && !is_live(R, R->nbr[i]))
			return 1;
	return b > a && R->nbr[b - 1] < 0;
}

static void
mark_patched(repair * R, int32_t e)
{
	if (!R->patched[e])
	{
		R->patched[e] = 1;
		R->patch_list[R->npatched++] = e;	/* (room: see apply_batch) */
	}
}

/* the searches and selections of a batch against the mirror as it stands, from entry point `from`; overflowed elements
 * are redone with dead_cap doubled */
static int
search_batch(repair * R, const int32_t *elems, int nb, int lcap, int32_t from)
{
	const int	stride = 2 * R->m;
	const int64_t per = (int64_t) lcap * stride;
	int64_t		want = (int64_t) nb * 2;
	int64_t		pairs = 0;
	int			cap = R->dead_cap;
	int			nover = 0;
	int			rc;

	/* the redo's outputs sit behind the batch's */
	if ((rc = ROOM(R, sel_ids, want * per)) != PGV_OK || (rc = ROOM(R, sel_dist, want * per)) != PGV_OK ||
		(rc = ROOM(R, sel_closer, want * per)) != PGV_OK || (rc = ROOM(R, sel_cnt, want * lcap)) != PGV_OK ||
		(rc = ROOM(R, status, want)) != PGV_OK || (rc = ROOM(R, redo, want)) != PGV_OK)
		return rc;

	/* RepairGraphElement's entryPoint argument: the entry-point step searches from the highest point */
	if ((rc = pgv_hnsw_update_graph(R->mirror, from, NULL, 0, NULL, NULL)) != PGV_OK)
		return rc;
	if ((rc = pgv_hnsw_repair_neighbors(R->mirror, elems, nb, R->efc, lcap, cap, R->sel_ids, R->sel_dist, R->sel_closer,
										R->sel_cnt, R->status, &pairs)) != PGV_OK)
		return rc;
	R->out->device_pairs += pairs;
	for (int q = 0; q < nb; q++)
		if (R->status[q])
			R->redo[nover++] = q;
	while (nover > 0)
	{
		int32_t    *r_elems = R->redo + nb;
		int32_t    *r_ids = R->sel_ids + (int64_t) nb * per;
		float	   *r_dist = R->sel_dist + (int64_t) nb * per;
		uint8_t    *r_closer = R->sel_closer + (int64_t) nb * per;
		int32_t    *r_cnt = R->sel_cnt + (int64_t) nb * lcap;
		int32_t    *r_status = R->status + nb;
		int			left = 0;

		if (cap >= R->dead_cap_max)
			return pgv_host_fail(PGV_ERR_NOMEM,
								 "pgv_host_hnsw_repair: the repair search of element %d holds more than %d dead elements in W, "
								 "all that fits the LDS at ef_construction %d / m %d",
								 (int) elems[R->redo[0]], cap, R->efc, R->m);
		cap = cap > 0 ? cap * 2 : 1;
		if (cap > R->dead_cap_max)
			cap = R->dead_cap_max;
		if (cap > R->out->dead_cap)
			R->out->dead_cap = cap;
		for (int i = 0; i < nover; i++)
			r_elems[i] = elems[R->redo[i]];
		if ((rc = pgv_hnsw_repair_neighbors(R->mirror, r_elems, nover, R->efc, lcap, cap, r_ids, r_dist, r_closer, r_cnt,
											r_status, &pairs)) != PGV_OK)
			return rc;
		R->out->device_pairs += pairs;
		R->out->overflow_redos += nover;
		for (int i = 0; i < nover; i++)
		{
			const int	q = R->redo[i];

			if (r_status[i])
			{
				R->redo[left++] = q;
				continue;
			}
			memcpy(R->sel_ids + (int64_t) q * per, r_ids + (int64_t) i * per, sizeof(int32_t) * (size_t) per);
			memcpy(R->sel_dist + (int64_t) q * per, r_dist + (int64_t) i * per, sizeof(float) * (size_t) per);
			memcpy(R->sel_cnt + (int64_t) q * lcap, r_cnt + (int64_t) i * lcap, sizeof(int32_t) * (size_t) lcap);
		}
		nover = left;
	}
	/* later batches start where this one had to go: deletes cluster, and a search run twice costs a search.  Up to
	 * DEAD_CAP_CARRY, below which W's 12 bytes an entry do not touch the kernel's occupancy */
	if (cap > R->dead_cap)
		R->dead_cap = cap < DEAD_CAP_CARRY ? cap : (R->dead_cap > DEAD_CAP_CARRY ? R->dead_cap : DEAD_CAP_CARRY);
	return PGV_OK;
}

static int
backlink_cmp(const void *pa, const void *pb)
{
	const backlink *a = pa,
			   *b = pb;

	if (a->owner != b->owner)
		return a->owner < b->owner ? -1 : 1;
	if (a->lc != b->lc)
		return a->lc < b->lc ? -1 : 1;
	return a->pos < b->pos ? -1 : (a->pos > b->pos ? 1 : 0);
}

/*
 * One list's back links, in element order, until one needs distances that are not here (returns 1: the list waits, its
 * group has been added to the round's request) or all are applied (0); a PGV_ERR_* code (> 1) when a selection fails.  UpdateNeighborOnDisk over GetUpdateIndex
 * (src/hnswinsert.c:409-540).
 */
static int
run_list(repair * R, listrun * run, int64_t *ngroups, int64_t *nids, int64_t *npairs)
{
	while (run->next < run->end)
	{
		const backlink *ev = &R->events[run->next];
		const int	lm = layer_m(R->m, ev->lc);
		int32_t    *list = R->nbr + R->nbr_start[ev->owner] + (int64_t) (R->levels[ev->owner] - ev->lc) * R->m;
		int			length = 0,
					exists = 0,
					idx = -1;

		if (R->levels[ev->owner] < ev->lc)
		{
			run->next++;		/* (an owner below the layer has no such list; the search never admits one) */
			continue;
		}
		while (length < lm && list[length] >= 0)
			length++;
		for (int i = 0; i < length; i++)
			exists |= list[i] == ev->e;
		if (exists)
			idx = -1;			/* ConnectionExists wins over everything */
		else if (length < lm)
			idx = length;		/* the first free slot */
		else
		{
			for (int i = 0; i < lm && idx < 0; i++)
				if (!is_live(R, list[i]))
					idx = i;	/* the first member being deleted, in list order */
			if (idx < 0)
			{
				if (run->tri_at < 0)
				{
					/* HnswUpdateConnection: the owner, its members and the newcomer meet on the device first */
					const int64_t g = *ngroups;
					int32_t    *ids = R->g_ids + *nids;

					ids[0] = ev->owner;
					memcpy(ids + 1, list, sizeof(int32_t) * (size_t) lm);
					ids[lm + 1] = ev->e;
					R->g_start[g] = *nids;
					R->g_from[g] = 1;
					R->g_pair[g] = *npairs;
					run->tri_at = *npairs;
					*nids += lm + 2;
					*npairs += (int64_t) (lm + 2) * (lm + 1) / 2;
					*ngroups = g + 1;
					return 1;
				}
				idx = pgv_host_hnsw_update_index(list, lm, ev->e, ev->dist, R->tri + run->tri_at);
				if (idx < -1)
					return pgv_host_fail(PGV_ERR_STATE, "pgv_host_hnsw_repair: the selection over element %d's list on layer %d "
										 "(%d members) failed", (int) ev->owner, (int) ev->lc, lm);
				run->tri_at = -1;
				R->out->reselections++;
			}
		}
		if (idx >= 0)
		{
			list[idx] = ev->e;
			mark_patched(R, ev->owner);
		}
		run->next++;
	}
	return 0;
}

/* the batch's own tuples and back links in element order, then the mirror's patch */
static int
apply_batch(repair * R, const int32_t *elems, int nb, int lcap)
{
	const int	m = R->m,
				stride = 2 * m;
	int			rc;
	double		t0 = now_secs(),
				t1;
	int64_t		maxlinks = 0;

	for (int q = 0; q < nb; q++)
	{
		R->pos_of[elems[q]] = q;
		maxlinks += (int64_t) (R->levels[elems[q]] + 2) * m;
	}
	if ((rc = ROOM(R, patch_list, nb + maxlinks)) != PGV_OK || (rc = ROOM(R, events, maxlinks)) != PGV_OK)
		return rc;
	R->npatched = 0;
	R->nevents = 0;
	/* HnswSetNeighborTuple: every layer's chosen neighbors, the rest of its slots invalid */
	for (int q = 0; q < nb; q++)
	{
		const int32_t e = elems[q];
		const int	level = R->levels[e];

		for (int lc = level; lc >= 0; lc--)
		{
			const int	lm = layer_m(m, lc);
			int32_t    *list = R->nbr + R->nbr_start[e] + (int64_t) (level - lc) * m;
			const int	cnt = lc < lcap ? R->sel_cnt[(int64_t) q * lcap + lc] : 0;
			const int32_t *ids = R->sel_ids + ((int64_t) q * lcap + (lc < lcap ? lc : 0)) * stride;
			const float *dist = R->sel_dist + ((int64_t) q * lcap + (lc < lcap ? lc : 0)) * stride;

			for (int i = 0; i < lm; i++)
				list[i] = i < cnt ? ids[i] : -1;
			for (int i = 0; i < cnt; i++)
			{
				const int32_t o = ids[i];
				backlink   *ev;

				/* (a link into a tuple that its owner's own repair overwrites later in the batch leaves no trace) */
				if (R->pos_of[o] > q)
					continue;
				ev = &R->events[R->nevents++];
				ev->owner = o;
				ev->lc = lc;
				ev->pos = q;
				ev->e = e;
				ev->dist = dist[i];
			}
		}
		mark_patched(R, e);
		R->out->repaired++;
	}
	for (int q = 0; q < nb; q++)
		R->pos_of[elems[q]] = -1;
	qsort(R->events, (size_t) R->nevents, sizeof(backlink), backlink_cmp);
	R->nruns = 0;
	if ((rc = ROOM(R, runs, R->nevents)) != PGV_OK)
		return rc;
	for (int64_t i = 0; i < R->nevents;)
	{
		int64_t		j = i + 1;

		while (j < R->nevents && R->events[j].owner == R->events[i].owner && R->events[j].lc == R->events[i].lc)
			j++;
		R->runs[R->nruns].next = i;
		R->runs[R->nruns].end = j;
		R->runs[R->nruns].tri_at = -1;
		R->nruns++;
		i = j;
	}
	/* rounds: every list as far as it gets without new distances; the waiting lists' pairs in one launch */
	{
		const int64_t gsize = stride + 2;

		if ((rc = ROOM(R, g_ids, R->nruns * gsize)) != PGV_OK || (rc = ROOM(R, g_start, R->nruns + 1)) != PGV_OK ||
			(rc = ROOM(R, g_from, R->nruns)) != PGV_OK || (rc = ROOM(R, g_pair, R->nruns + 1)) != PGV_OK)
			return rc;
	}
	for (int64_t waiting = R->nruns; waiting > 0;)
	{
		int64_t		ngroups = 0,
					nids = 0,
					npairs = 0;

		waiting = 0;
		for (int64_t k = 0; k < R->nruns; k++)
			if (R->runs[k].next < R->runs[k].end)
			{
				const int	w = run_list(R, &R->runs[k], &ngroups, &nids, &npairs);

				if (w > 1)
					return w;
				waiting += w;
			}
		if (ngroups == 0)
			break;
		R->g_start[ngroups] = nids;
		R->g_pair[ngroups] = npairs;
		if ((rc = ROOM(R, tri, npairs)) != PGV_OK)
			return rc;
		t1 = now_secs();
		R->out->phase_secs[1] += t1 - t0;
		if ((rc = pgv_hnsw_score_groups(R->mirror, R->g_ids, R->g_start, R->g_from, R->g_pair, (int) ngroups, nids, npairs,
										R->tri)) != PGV_OK)
			return rc;
		t0 = now_secs();
		R->out->phase_secs[2] += t0 - t1;
		R->out->device_pairs += npairs;
	}
	t1 = now_secs();
	R->out->phase_secs[1] += t1 - t0;
	/* the changed tuples whole, as pgv_hnsw_update_graph takes them */
	{
		int64_t		total = 0;

		for (int64_t i = 0; i < R->npatched; i++)
			total += R->nbr_start[R->patch_list[i] + 1] - R->nbr_start[R->patch_list[i]];
		if ((rc = ROOM(R, tup, total)) != PGV_OK || (rc = ROOM(R, tup_off, R->npatched + 1)) != PGV_OK)
			return rc;
		total = 0;
		for (int64_t i = 0; i < R->npatched; i++)
		{
			const int32_t e = R->patch_list[i];
			const int64_t len = R->nbr_start[e + 1] - R->nbr_start[e];

			R->tup_off[i] = total;
			memcpy(R->tup + total, R->nbr + R->nbr_start[e], sizeof(int32_t) * (size_t) len);
			total += len;
			R->patched[e] = 0;
		}
		R->tup_off[R->npatched] = total;
	}
	rc = pgv_hnsw_update_graph(R->mirror, R->entry, R->patch_list, (int) R->npatched, R->tup_off, R->tup);
	R->out->phase_secs[3] += now_secs() - t1;
	R->out->batches++;
	return rc;
}

/* RepairGraphElement for a batch: searched from `from`, applied; the graph's entry point is R->entry afterwards */
static int
repair_elements(repair * R, const int32_t *elems, int nb, int32_t from)
{
	int			lcap = 1;
	int			rc;
	double		t0 = now_secs();

	for (int q = 0; q < nb; q++)
		if (R->levels[elems[q]] + 1 > lcap)
			lcap = R->levels[elems[q]] + 1;
	rc = search_batch(R, elems, nb, lcap, from);
	R->out->phase_secs[0] += now_secs() - t0;
	if (rc != PGV_OK)
		return rc;
	return apply_batch(R, elems, nb, lcap);
}

void
pgv_host_hnsw_repaired_free(pgv_hnsw_repaired * r)
{
	if (!r)
		return;
	free(r->nbr);
	memset(r, 0, sizeof(*r));
}

int
pgv_host_hnsw_repair(pgv_hnsw * mirror, int64_t n, const int32_t *levels, const int64_t *nbr_start, const int32_t *nbr,
					 int32_t entry, const uint32_t *live, int m, int ef_construction, int max_batch, int dead_cap,
					 pgv_hnsw_repaired * out)
{
	repair		R;
	int			rc = PGV_OK;
	int32_t		highest = -1,
				fallback = -1;
	int			highest_level = -1,
				fallback_level = -1;
	int32_t    *batch = NULL;

	if (!mirror || !out || !levels || !nbr_start || !nbr || !live)
		return pgv_host_fail(PGV_ERR_ARG, "pgv_host_hnsw_repair: mirror/graph/live/out is NULL");
	memset(out, 0, sizeof(*out));
	if (!pgv_hnsw_set_live || !pgv_hnsw_repair_neighbors || !pgv_hnsw_repair_dead_cap_max)
		return pgv_host_fail(PGV_ERR_STATE, "pgv_host_hnsw_repair: the device library has no pgv_hnsw_set_live / "
							 "pgv_hnsw_repair_neighbors");
	if (n < 1 || n > 0x7fffffff || m < 2 || m > 100 || entry < -1 || entry >= n || max_batch < 1 || dead_cap < 0)
		return pgv_host_fail(PGV_ERR_ARG, "pgv_host_hnsw_repair: bad sizes (n %lld, m %d, entry %d, max_batch %d, dead_cap %d)",
							 (long long) n, m, (int) entry, max_batch, dead_cap);
	if (ef_construction < 4 || ef_construction > 1000)
		return pgv_host_fail(PGV_ERR_ARG, "ef_construction must be 4..1000 (src/hnsw.h:58-59), got %d", ef_construction);
	for (int64_t e = 0; e < n; e++)
		if (levels[e] < 0 || nbr_start[e + 1] - nbr_start[e] != (int64_t) (levels[e] + 2) * m)
			return pgv_host_fail(PGV_ERR_ARG, "pgv_host_hnsw_repair: element %lld's tuple is not (level + 2) * m slots",
								 (long long) e);
	memset(&R, 0, sizeof(R));
	R.mirror = mirror;
	R.n = n;
	R.levels = levels;
	R.nbr_start = nbr_start;
	R.live = live;
	R.m = m;
	R.efc = ef_construction;
	R.entry = entry;
	R.out = out;
	out->nbr_total = nbr_start[n];
	for (int64_t i = 0; i < out->nbr_total; i++)
		if (nbr[i] >= n)
			return pgv_host_fail(PGV_ERR_ARG, "pgv_host_hnsw_repair: neighbor slot %lld names element %d of %lld", (long long) i,
								 (int) nbr[i], (long long) n);
	/* the mirror holds this graph and this bitmap from here on */
	if ((rc = pgv_hnsw_set_graph(mirror, m, entry, levels, nbr_start, nbr)) != PGV_OK)
		return rc;
	if ((rc = pgv_hnsw_set_live(mirror, live, (n + 31) / 32)) != PGV_OK)
		return rc;
	R.dead_cap_max = pgv_hnsw_repair_dead_cap_max(mirror, ef_construction);
	if (R.dead_cap_max < 0)
		return pgv_host_fail(PGV_ERR_ARG, "pgv_host_hnsw_repair: ef_construction %d / m %d do not fit the LDS", ef_construction, m);
	R.dead_cap = dead_cap > 0 ? dead_cap : 64;
	if (R.dead_cap > R.dead_cap_max)
		R.dead_cap = R.dead_cap_max;
	out->dead_cap = R.dead_cap;
	R.nbr = malloc(sizeof(int32_t) * (size_t) (out->nbr_total > 0 ? out->nbr_total : 1));
	R.pos_of = malloc(sizeof(int32_t) * (size_t) n);
	R.patched = calloc((size_t) n, 1);
	batch = malloc(sizeof(int32_t) * (size_t) max_batch);
	if (!R.nbr || !R.pos_of || !R.patched || !batch)
	{
		rc = pgv_host_fail(PGV_ERR_NOMEM, "pgv_host_hnsw_repair: out of host memory");
		goto done;
	}
	memcpy(R.nbr, nbr, sizeof(int32_t) * (size_t) out->nbr_total);
	for (int64_t e = 0; e < n; e++)
		R.pos_of[e] = -1;

	/* RemoveHeapTids' highest and fallback point (src/hnswvacuum.c:133-157), over the live elements in slot order */
	for (int64_t e = 0; e < n; e++)
	{
		if (!is_live(&R, (int32_t) e))
			continue;
		if (levels[e] > highest_level)
		{
			if (highest >= 0)
			{
				fallback = highest;
				fallback_level = highest_level;
			}
			highest = (int32_t) e;
			highest_level = levels[e];
		}
		else if (levels[e] > fallback_level)
		{
			fallback = (int32_t) e;
			fallback_level = levels[e];
		}
	}
	/* RepairGraphEntryPoint (:280-373) */
	if (highest >= 0)
	{
		if (R.entry == highest)
			highest = fallback;
		if (highest >= 0 && needs_updated(&R, highest) && (rc = repair_elements(&R, &highest, 1, R.entry)) != PGV_OK)
			goto done;
	}
	if (R.entry >= 0)
	{
		if (!is_live(&R, R.entry))
		{
			R.entry = highest;
			if ((rc = pgv_hnsw_update_graph(mirror, R.entry, NULL, 0, NULL, NULL)) != PGV_OK)
				goto done;
		}
		else if (needs_updated(&R, R.entry))
		{
			const int32_t ep = R.entry;

			if ((rc = repair_elements(&R, &ep, 1, highest)) != PGV_OK)
				goto done;
		}
	}
	/* every live element in slot order (:395-501) */
	for (int64_t cursor = 0; cursor < n;)
	{
		int			nb = 0;
		int			tall = 0;

		if (pgv_host_hnsw_cancelled())
		{
			rc = pgv_host_fail(PGV_ERR_STATE, "pgv_host_hnsw_repair: cancelled after %lld of %lld elements", (long long) cursor,
							   (long long) n);
			goto done;
		}
		while (cursor < n && nb < max_batch)
		{
			const int32_t e = (int32_t) cursor;

			if (is_live(&R, e))
			{
				const int	is_tall = R.entry < 0 || levels[e] > levels[R.entry];

				/* (NeedsUpdated, then RepairGraphElement's own test: the entry point is left alone, :241-242) */
				if (e != R.entry && needs_updated(&R, e))
				{
					if (is_tall && nb > 0)
						break;	/* a batch ends before an element taller than the entry point */
					batch[nb++] = e;
					tall = is_tall;
				}
				out->examined++;
			}
			cursor++;
			if (tall)
				break;
		}
		if (nb == 0)
			continue;
		if (tall)
		{
			/* the exclusive path (:460-482): repaired against the old entry point, then it is the entry point */
			const int32_t from = R.entry;

			R.entry = batch[0];
			rc = repair_elements(&R, batch, 1, from);
		}
		else
			rc = repair_elements(&R, batch, nb, R.entry);
		if (rc != PGV_OK)
			goto done;
	}
	out->entry = R.entry;
	out->nbr = R.nbr;
	R.nbr = NULL;
done:
	free(R.nbr);
	free(R.pos_of);
	free(R.patched);
	free(batch);
	free(R.sel_ids);
	free(R.sel_dist);
	free(R.sel_closer);
	free(R.sel_cnt);
	free(R.status);
	free(R.redo);
	free(R.patch_list);
	free(R.events);
	free(R.runs);
	free(R.g_ids);
	free(R.g_start);
	free(R.g_from);
	free(R.g_pair);
	free(R.tri);
	free(R.tup_off);
	free(R.tup);
	if (rc != PGV_OK)
		memset(out, 0, sizeof(*out));
	return rc;
}
