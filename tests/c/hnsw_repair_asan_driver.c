/*
 * hnsw_repair_asan_driver.c -- pgv_host_hnsw_repair's host logic (pgvector_amd/host/hnsw_repair.c: the batches, the
 * overflow redo, the back-link replay with its rounds of pair scoring, the patch) run as a program of its own, for
 * -fsanitize=address,undefined (tests/test_hnsw_repair_asan_cpu.py).
 *
 * The device is tests/c/mock_hip.c, whose "repair search" is no model of the device's (tests/hnsw_repair_model.py and the
 * GPU tests are): it feeds the host driver lists of the right shape, which is what its buffers are sized by, and lets
 * every fifth element overflow so that the redo path runs with several doublings.  The graph is hnsw_repair_scenario.h's.
 *
 * usage: hnsw_repair_asan_driver <n> <max_batch> [<max_batch> ...]; prints "rc 0 ..." per run, exits nonzero on any error
 * or broken invariant.
 */
#include "hnsw_repair_scenario.h"

#include <stdio.h>

int
main(int argc, char **argv)
{
	repair_scenario s;
	int			bad = 0;

	if (argc < 3)
		return 2;
	if (repair_scenario_make(&s, atoll(argv[1]), 0))
		return 3;
	for (int a = 2; a < argc; a++)
	{
		pgv_hnsw_repaired out;
		const int	rc = pgv_host_hnsw_repair(s.h, s.n, s.levels, s.start, s.nbr, s.entry, s.live, RS_M, 8, atoi(argv[a]), 2, &out);

		if (rc != PGV_OK)
		{
			printf("max_batch %s: rc %d %s\n", argv[a], rc, pgv_host_last_error());
			bad = 1;
			continue;
		}
		bad |= repair_scenario_broken(&s, &out);
		printf("rc 0 max_batch %s: repaired %lld batches %lld redos %lld reselections %lld dead_cap %d entry %d%s\n", argv[a],
			   (long long) out.repaired, (long long) out.batches, (long long) out.overflow_redos, (long long) out.reselections,
			   (int) out.dead_cap, (int) out.entry, bad ? " BROKEN" : "");
		pgv_host_hnsw_repaired_free(&out);
	}
	repair_scenario_free(&s);
	return bad;
}
