/*
 * hnsw_host.h -- what the HNSW host files (hnsw_build.c, hnsw_repair.c) share.  Internal: not installed, not part of
 * pgv_host.h.
 */
#ifndef PGV_HNSW_HOST_H
#define PGV_HNSW_HOST_H

#include "pgv_host.h"

#include <stdlib.h>
#include <string.h>
#include <time.h>

/* sets pgv_host_last_error's text and returns code (hnsw_search.c) */
int			pgv_host_fail(int code, const char *fmt,...);

/*
 * HnswUpdateConnection on a full list read back from its tuple (hnsw_build.c, with SelectNeighbors): the index of the
 * member the newcomer replaces, -1 when the newcomer itself is pruned, -2 when the selection could not be made.
 */
int			pgv_host_hnsw_update_index(const int32_t *members, int lm, int32_t newcomer, float new_dist, const float *tri);

/* nonzero when the callback of pgv_host_hnsw_set_cancel_check asks this thread's build or repair to stop (hnsw_build.c) */
int			pgv_host_hnsw_cancelled(void);

static inline double
now_secs(void)
{
	struct timespec ts;

	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (double) ts.tv_sec + 1e-9 * (double) ts.tv_nsec;
}

static inline int
layer_m(int m, int lc)
{
	return lc == 0 ? 2 * m : m; /* HnswGetLayerM, src/hnsw.h:127 */
}

/* room for `want` items in the array whose pointer (of any item type) is at `arr` and which has room for *cap: grown by
 * doubling and moved if need be.  0 = out of memory (the array stays as it was) */
static inline int
grow(void *arr, int64_t *cap, int64_t want, size_t item_bytes)
{
	void	   *p;
	int64_t		c = *cap < 64 ? 64 : *cap;

	if (want <= *cap)
		return 1;
	while (c < want)
		c *= 2;
	memcpy(&p, arr, sizeof(p));
	if (!(p = realloc(p, (size_t) c * item_bytes)))
		return 0;
	memcpy(arr, &p, sizeof(p));
	*cap = c;
	return 1;
}

/* ------------------------------------------------------------ pair requests */

/* a request to pgv_hnsw_score_groups: lists of element slots and, per list, which of its pairs are wanted */
typedef struct
{
	int32_t    *ids;
	int64_t    *ids_start;		/* [ngroups + 1] */
	int32_t    *from;			/* [ngroups] */
	int64_t    *pair_start;		/* [ngroups + 1] */
	int64_t		nids,
				ngroups;
	int64_t		ids_cap,
				ids_start_cap,
				from_cap,
				pair_start_cap;
}			groupbuf;

static inline void
groups_reset(groupbuf * gb)
{
	gb->nids = 0;
	gb->ngroups = 0;
}

/* pairs (u, v), v < u, of the locals u >= from of ids[0 .. n): they start at pair0 in the reply.  0 = out of memory */
static inline int
groups_add(groupbuf * gb, const int32_t *ids, int n, int from, int64_t pair0)
{
	const int64_t g = gb->ngroups;

	if (!grow(&gb->ids, &gb->ids_cap, gb->nids + n, sizeof(int32_t)) ||
		!grow(&gb->ids_start, &gb->ids_start_cap, g + 2, sizeof(int64_t)) ||
		!grow(&gb->from, &gb->from_cap, g + 1, sizeof(int32_t)) ||
		!grow(&gb->pair_start, &gb->pair_start_cap, g + 2, sizeof(int64_t)))
		return 0;
	memcpy(gb->ids + gb->nids, ids, sizeof(int32_t) * (size_t) n);
	gb->ids_start[g] = gb->nids;
	gb->from[g] = from;
	gb->pair_start[g] = pair0;
	gb->nids += n;
	gb->ids_start[g + 1] = gb->nids;
	gb->ngroups = g + 1;
	return 1;
}

/* pairs a group (n locals, from) asks for */
static inline int64_t
group_pairs(int n, int from)
{
	if (from < 1)
		from = 1;
	return n > from ? ((int64_t) n * (n - 1) - (int64_t) from * (from - 1)) / 2 : 0;
}

/* the request is complete: npairs pairs in all */
static inline void
groups_end(groupbuf * gb, int64_t npairs)
{
	if (gb->ngroups > 0)
		gb->pair_start[gb->ngroups] = npairs;
}

static inline void
groups_free(groupbuf * gb)
{
	free(gb->ids);
	free(gb->ids_start);
	free(gb->from);
	free(gb->pair_start);
	memset(gb, 0, sizeof(*gb));
}

/* the distances a request asks for, on `handle` (the mirror, or a helper's view of it) */
static inline int
score_groups(pgv_hnsw * handle, const groupbuf * gb, int64_t npairs, float *out)
{
	return pgv_hnsw_score_groups(handle, gb->ids, gb->ids_start, gb->from, gb->pair_start, (int) gb->ngroups, gb->nids, npairs,
								 out);
}

#endif
