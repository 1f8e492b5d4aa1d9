/* bh_cluster.c as a stand-alone program (built by tests/test_cluster_cpu.py with the address and undefined-behaviour sanitizers): the name
 * table, a .b6 file, the yardstick behind the solver hook, the two tables, a duplicate name, a random graph.  The device entry points
 * are stubs: nothing here reaches them. */
#include "burst_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int bhip_cluster_run(void *h, uint32_t n, const uint32_t *w, const BhipClusterEdge *e, uint64_t m, uint32_t *c, uint32_t *d) { (void)h;(void)n;(void)w;(void)e;(void)m;(void)c;(void)d; return -2; }
int bhip_cluster_info(void *h, uint64_t info[8]) { (void)h; memset(info, 0, 64); return 0; }
const char *bhip_last_error(void) { return "stub"; }
int main(int argc, char **argv) {
	if (argc < 3) return 9;
	const char *names[] = {"a;size=3", "b;size=10;", "c", "d;size=3", "lonely", "e;size=x", "f;size=2;extra", ""};
	for (int sizes = 0; sizes < 2; ++sizes) {
		BhCluster *cl = NULL;
		if (bh_cluster_open(argv[1], sizes, &cl)) return 1;
		bh_cluster_set_solver(cl, bh_cluster_host, NULL);
		if (bh_cluster_names(cl, names, 8)) return 2;
		if (bh_cluster_add_b6(cl, argv[2])) { puts(bh_last_error()); return 3; }
		if (bh_cluster_solve(cl, NULL) || bh_cluster_write(cl)) return 4;
		bh_cluster_print_info(cl);
		bh_cluster_close(cl);
	}
	BhCluster *cl = NULL; bh_cluster_open(argv[1], 0, &cl);
	const char *dup[] = {"x", "y", "x"};
	if (bh_cluster_names(cl, dup, 3) == 0) return 5;
	puts(bh_last_error());
	bh_cluster_close(cl);
	/* a random graph through the yardstick */
	uint32_t n = 5000, *w = malloc(n * 4), *c = malloc(n * 4), *d = malloc(n * 4); uint64_t m = 60000; BhipClusterEdge *e = malloc(m * sizeof *e);
	srand(1);
	for (uint32_t i = 0; i < n; ++i) w[i] = 1 + rand() % 4;
	for (uint64_t i = 0; i < m; ++i) { e[i].q = rand() % n; e[i].r = rand() % n; e[i].edits = rand() % 5; }
	uint64_t info[8];
	if (bh_cluster_host(NULL, n, w, e, m, c, d, info)) return 6;
	if (bh_cluster_host(NULL, 0, NULL, NULL, 0, NULL, NULL, info)) return 7;
	printf("cluster_host_main ok\n");
	free(w); free(c); free(d); free(e);
	return 0;
}
