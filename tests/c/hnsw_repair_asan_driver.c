/*
 * hnsw_repair_asan_driver.c -- pgv_host_hnsw_repair's host logic (pgvector_amd/host/hnsw_repair.c: the batches, the
 * overflow redo, the back-link replay with its rounds of pair scoring, the patch) run as a program of its own, for
 * -fsanitize=address,undefined (tests/test_hnsw_repair_asan_cpu.py).
 *
 * The device is tests/c/mock_hip.c for everything it has (the mirror, pgv_hnsw_set_graph, pgv_hnsw_update_graph,
 * pgv_hnsw_score_groups).  The three vacuum-side entries it lacks are stood in for HERE -- hnsw_repair.c references them
 * weakly -- by something much simpler than the device's search: an element's "repair search" answers, on every layer, the
 * nearest live elements of that layer by brute force, furthest first; every fifth element overflows any dead_cap below
 * 100, so the redo path runs with several doublings.  That is no model of the search (tests/hnsw_repair_model.py and the
 * GPU tests are); it feeds the host driver lists of the right shape, which is what its buffers are sized by.
 *
 * usage: hnsw_repair_asan_driver <n> <max_batch> [<max_batch> ...]; prints "rc 0 ..." per run, exits nonzero on any error
 * or broken invariant.
 */
#include "pgv_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define DIM 8
#define M 4

static int64_t g_n;
static float *g_rows;
static int32_t *g_levels;
static const uint32_t *g_live;

static uint32_t g_seed = 12345;
static uint32_t
rnd(void)
{
	g_seed = g_seed * 1664525u + 1013904223u;
	return g_seed >> 8;
}

static float
sqdist(int64_t a, int64_t b)
{
	float		s = 0;

	for (int i = 0; i < DIM; i++)
	{
		const float d = g_rows[a * DIM + i] - g_rows[b * DIM + i];

		s += d * d;
	}
	return s;
}

static int
is_live(int64_t e)
{
	return !g_live || ((g_live[e >> 5] >> (e & 31)) & 1u);
}

/* the lm nearest elements x != e with levels[x] >= lc (and live, if asked), nearest first; returns how many */
static int
nearest(int64_t e, int lc, int lm, int only_live, int32_t *ids, float *dist)
{
	int			cnt = 0;

	for (int64_t x = 0; x < g_n; x++)
	{
		float		d;
		int			j;

		if (x == e || g_levels[x] < lc || (only_live && !is_live(x)))
			continue;
		d = sqdist(e, x);
		if (cnt == lm && d >= dist[cnt - 1])
			continue;
		j = cnt < lm ? cnt++ : lm - 1;
		while (j > 0 && dist[j - 1] > d)
		{
			dist[j] = dist[j - 1];
			ids[j] = ids[j - 1];
			j--;
		}
		dist[j] = d;
		ids[j] = (int32_t) x;
	}
	return cnt;
}

/* ---- the entries tests/c/mock_hip.c does not have */

int
pgv_hnsw_set_live(pgv_hnsw * h, const uint32_t *live, int64_t words)
{
	(void) h;
	if (live && words != (g_n + 31) / 32)
		return PGV_ERR_ARG;
	g_live = live;
	return PGV_OK;
}

int64_t
pgv_hnsw_live_count(const pgv_hnsw * h)
{
	int64_t		c = 0;

	(void) h;
	for (int64_t e = 0; e < g_n; e++)
		c += is_live(e);
	return c;
}

int
pgv_hnsw_repair_dead_cap_max(const pgv_hnsw * h, int ef_construction)
{
	(void) h;
	(void) ef_construction;
	return 4096;
}

int
pgv_hnsw_repair_neighbors(pgv_hnsw * h, const int32_t *elements, int nq, int ef_construction, int layer_cap, int dead_cap,
						  int32_t *out_ids, float *out_dist, uint8_t *out_closer, int32_t *out_count, int32_t *out_status,
						  int64_t *out_pairs)
{
	const int	stride = 2 * M;

	(void) h;
	(void) ef_construction;
	if (out_pairs)
		*out_pairs = 0;
	for (int q = 0; q < nq; q++)
	{
		const int32_t e = elements[q];

		out_status[q] = dead_cap < (e % 5 == 0 ? 100 : 3);
		for (int lc = 0; lc < layer_cap; lc++)
		{
			int32_t		ids[2 * M];
			float		dist[2 * M];
			const size_t o = ((size_t) q * layer_cap + lc) * stride;
			int			cnt = 0;

			if (!out_status[q] && lc <= g_levels[e])
				cnt = nearest(e, lc, lc == 0 ? 2 * M : M, 1, ids, dist);
			out_count[(size_t) q * layer_cap + lc] = cnt;
			for (int i = 0; i < cnt; i++)	/* furthest first, as a list taken whole */
			{
				out_ids[o + i] = ids[cnt - 1 - i];
				out_dist[o + i] = dist[cnt - 1 - i];
				out_closer[o + i] = 0;
			}
		}
	}
	return PGV_OK;
}

int
main(int argc, char **argv)
{
	pgv_ctx    *ctx = NULL;
	pgv_hnsw   *h = NULL;
	int64_t    *start;
	int32_t    *nbr;
	uint32_t   *live;
	int32_t		entry = 0;
	int			bad = 0;

	if (argc < 3)
		return 2;
	g_n = atoll(argv[1]);
	g_rows = malloc(sizeof(float) * (size_t) g_n * DIM);
	g_levels = malloc(sizeof(int32_t) * (size_t) g_n);
	start = malloc(sizeof(int64_t) * (size_t) (g_n + 1));
	live = calloc((size_t) (g_n + 31) / 32, sizeof(uint32_t));
	start[0] = 0;
	for (int64_t e = 0; e < g_n; e++)
	{
		const uint32_t r = rnd() & 63;

		for (int i = 0; i < DIM; i++)
			g_rows[e * DIM + i] = (float) ((int) (rnd() % 1401) - 700);
		g_levels[e] = r == 0 ? 2 : (r < 12 ? 1 : 0);
		if (g_levels[e] > g_levels[entry])
			entry = (int32_t) e;
		start[e + 1] = start[e] + (int64_t) (g_levels[e] + 2) * M;
		if (rnd() % 4 != 0)
			live[e >> 5] |= 1u << (e & 31);
	}
	nbr = malloc(sizeof(int32_t) * (size_t) start[g_n]);
	for (int64_t i = 0; i < start[g_n]; i++)
		nbr[i] = -1;
	g_live = NULL;
	for (int64_t e = 0; e < g_n; e++)
		for (int lc = 0; lc <= g_levels[e]; lc++)
		{
			float		dist[2 * M];

			/* (every seventh element's lists one short: NeedsUpdated's second reason, and the free-slot rule) */
			nearest(e, lc, (lc == 0 ? 2 * M : M) - (e % 7 == 0), 0, nbr + start[e] + (int64_t) (g_levels[e] - lc) * M, dist);
		}
	if (pgv_ctx_create(0, NULL, &ctx) != PGV_OK ||
		pgv_hnsw_upload(ctx, PGV_L2SQ, PGV_F32, DIM, g_rows, g_n, &h) != PGV_OK)
		return 3;
	for (int a = 2; a < argc; a++)
	{
		pgv_hnsw_repaired out;
		const int	rc = pgv_host_hnsw_repair(h, g_n, g_levels, start, nbr, entry, live, M, 8, atoi(argv[a]), 2, &out);

		if (rc != PGV_OK)
		{
			printf("max_batch %s: rc %d %s\n", argv[a], rc, pgv_host_last_error());
			bad = 1;
			continue;
		}
		g_live = live;
		for (int64_t e = 0; e < g_n; e++)
			for (int64_t i = start[e]; is_live(e) && i < start[e + 1]; i++)
				if (out.nbr[i] >= g_n || (out.nbr[i] >= 0 && !is_live(out.nbr[i])))
					bad = 1;
		if (out.entry >= 0 && !is_live(out.entry))
			bad = 1;
		printf("rc 0 max_batch %s: repaired %lld batches %lld redos %lld reselections %lld dead_cap %d entry %d%s\n", argv[a],
			   (long long) out.repaired, (long long) out.batches, (long long) out.overflow_redos, (long long) out.reselections,
			   (int) out.dead_cap, (int) out.entry, bad ? " BROKEN" : "");
		pgv_host_hnsw_repaired_free(&out);
	}
	pgv_hnsw_free(h);
	pgv_ctx_destroy(ctx);
	free(nbr);
	free(live);
	free(start);
	free(g_levels);
	free(g_rows);
	return bad;
}
