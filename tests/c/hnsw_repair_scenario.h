/*
 * hnsw_repair_scenario.h -- the graph that the CPU programs of pgv_host_hnsw_repair repair on tests/c/mock_hip.c
 * (hnsw_repair_asan_driver.c, host_logic_driver.c): n elements of RS_DIM integer coordinates on three levels, every list
 * the nearest elements of its layer (every seventh element's lists one short: NeedsUpdated's second reason, and the
 * free-slot rule), a quarter of the elements dead.  The lists are the mock's own brute-force answers
 * (pgv_hnsw_repair_neighbors with nothing marked dead), so the repair's searches and the graph agree on what is near.
 */
#include "pgv_host.h"

#include <stdlib.h>

#define RS_DIM 8
#define RS_M 4

typedef struct
{
	int64_t		n;
	float	   *rows;
	int32_t    *levels;
	int64_t    *start;
	int32_t    *nbr;
	uint32_t   *live;
	int32_t		entry;
	pgv_ctx    *ctx;
	pgv_hnsw   *h;
}			repair_scenario;

static uint32_t rs_seed;

static uint32_t
rs_rnd(void)
{
	rs_seed = rs_seed * 1664525u + 1013904223u;
	return rs_seed >> 8;
}

static void
repair_scenario_free(repair_scenario * s)
{
	pgv_hnsw_free(s->h);
	pgv_ctx_destroy(s->ctx);
	free(s->nbr);
	free(s->live);
	free(s->start);
	free(s->levels);
	free(s->rows);
}

/* every_fourth: elements 3, 7, 11, ... are dead; otherwise a random quarter.  Nonzero when it could not be made */
static int
repair_scenario_make(repair_scenario * s, int64_t n, int every_fourth)
{
	const int	stride = 2 * RS_M,
				lcap = 3;
	int32_t    *all = malloc(sizeof(int32_t) * (size_t) n),
			   *ids = malloc(sizeof(int32_t) * (size_t) n * lcap * stride),
			   *cnt = malloc(sizeof(int32_t) * (size_t) n * lcap),
			   *status = malloc(sizeof(int32_t) * (size_t) n);
	float	   *dist = malloc(sizeof(float) * (size_t) n * lcap * stride);
	uint8_t    *closer = malloc((size_t) n * lcap * stride);
	int			rc;

	rs_seed = 12345;
	s->n = n;
	s->entry = 0;
	s->rows = malloc(sizeof(float) * (size_t) n * RS_DIM);
	s->levels = malloc(sizeof(int32_t) * (size_t) n);
	s->start = malloc(sizeof(int64_t) * (size_t) (n + 1));
	s->live = calloc((size_t) (n + 31) / 32, sizeof(uint32_t));
	s->start[0] = 0;
	for (int64_t e = 0; e < n; e++)
	{
		const uint32_t r = rs_rnd() & 63;

		for (int i = 0; i < RS_DIM; i++)
			s->rows[e * RS_DIM + i] = (float) ((int) (rs_rnd() % 1401) - 700);
		s->levels[e] = r == 0 ? 2 : (r < 12 ? 1 : 0);
		if (s->levels[e] > s->levels[s->entry])
			s->entry = (int32_t) e;
		s->start[e + 1] = s->start[e] + (int64_t) (s->levels[e] + 2) * RS_M;
		if (every_fourth ? e % 4 != 3 : rs_rnd() % 4 != 0)
			s->live[e >> 5] |= 1u << (e & 31);
		all[e] = (int32_t) e;
	}
	s->nbr = malloc(sizeof(int32_t) * (size_t) s->start[n]);
	for (int64_t i = 0; i < s->start[n]; i++)
		s->nbr[i] = -1;
	rc = pgv_ctx_create(0, NULL, &s->ctx) != PGV_OK ||
		pgv_hnsw_upload(s->ctx, PGV_L2SQ, PGV_F32, RS_DIM, s->rows, n, &s->h) != PGV_OK ||
		pgv_hnsw_set_graph(s->h, RS_M, s->entry, s->levels, s->start, s->nbr) != PGV_OK ||
		pgv_hnsw_repair_neighbors(s->h, all, (int) n, 8, lcap, 4096, ids, dist, closer, cnt, status, NULL) != PGV_OK;
	for (int64_t e = 0; !rc && e < n; e++)
		for (int lc = 0; lc <= s->levels[e]; lc++)
		{
			const int64_t o = (e * lcap + lc) * stride;
			const int	len = cnt[e * lcap + lc] - (e % 7 == 0 && cnt[e * lcap + lc] == (lc == 0 ? stride : RS_M));

			/* (the answers come furthest first; a tuple holds them nearest first) */
			for (int i = 0; i < len; i++)
				s->nbr[s->start[e] + (int64_t) (s->levels[e] - lc) * RS_M + i] = ids[o + cnt[e * lcap + lc] - 1 - i];
		}
	free(all);
	free(ids);
	free(cnt);
	free(status);
	free(dist);
	free(closer);
	return rc;
}

static int
rs_is_live(const repair_scenario * s, int64_t e)
{
	return (s->live[e >> 5] >> (e & 31)) & 1u;
}

/* what every repair must leave behind: no live element's tuple names a dead element, and the entry point is live */
static int
repair_scenario_broken(const repair_scenario * s, const pgv_hnsw_repaired * out)
{
	for (int64_t e = 0; e < s->n; e++)
		for (int64_t i = s->start[e]; rs_is_live(s, e) && i < s->start[e + 1]; i++)
			if (out->nbr[i] >= s->n || (out->nbr[i] >= 0 && !rs_is_live(s, out->nbr[i])))
				return 1;
	return out->entry >= 0 && !rs_is_live(s, out->entry);
}
