/* bh_chimera.c as a stand-alone program (built by tests/test_chimera_cpu.py with the address and undefined-behaviour sanitizers): the
 * reads, a .b6 file with the path columns, the yardstick behind the solver hook, the table, a duplicate name, bad arguments.  The device
 * entry points and the path tracer's hook are stubs: nothing here reaches them. */
#include "burst_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int bhip_cluster_run(void *h, uint32_t n, const uint32_t *w, const BhipClusterEdge *e, uint64_t m, uint32_t *c, uint32_t *d) { (void)h;(void)n;(void)w;(void)e;(void)m;(void)c;(void)d; return -2; }
int bhip_cluster_info(void *h, uint64_t info[8]) { (void)h; memset(info, 0, 64); return 0; }
int bhip_chimera_run(void *h, uint32_t n, const uint32_t *w, const uint32_t *len, const BhipChimLine *l, uint64_t m, const uint32_t *ops, uint64_t n_ops, uint32_t s, uint32_t g,
                     uint32_t d, BhipChimera *out) { (void)h;(void)n;(void)w;(void)len;(void)l;(void)m;(void)ops;(void)n_ops;(void)s;(void)g;(void)d;(void)out; return -2; }
int bhip_chimera_info(void *h, uint64_t info[8]) { (void)h; memset(info, 0, 64); return 0; }
const char *bhip_last_error(void) { return "stub"; }
void bh_paths_set_collector(BhPaths *p, bh_paths_collect_fn fn, void *ctx, int columns) { (void)p;(void)fn;(void)ctx;(void)columns; }
int main(int argc, char **argv) {
	if (argc < 3) return 9;
	const char *names[] = {"q;size=1", "a;size=9", "b;size=9;", "lonely", "n;size=4", "c"};
	const uint32_t lens[] = {40, 40, 40, 40, 40, 40};
	for (int sizes = 0; sizes < 2; ++sizes) {
		BhChimera *ch = NULL;
		if (bh_chimera_open(argv[1], sizes, 2, 16, 3, &ch)) return 1;
		bh_chimera_set_solver(ch, bh_chimera_host, NULL);
		if (bh_chimera_names(ch, names, lens, 6)) return 2;
		if (bh_chimera_add_b6(ch, argv[2])) { puts(bh_last_error()); return 3; }
		if (bh_chimera_solve(ch, NULL) || bh_chimera_write(ch)) { puts(bh_last_error()); return 4; }
		bh_chimera_print_info(ch);
		bh_chimera_close(ch);
	}
	BhChimera *ch = NULL;
	if (bh_chimera_open(argv[1], 0, 2, 16, 3, &ch)) return 5;
	const char *dup[] = {"x", "y", "x"};
	if (bh_chimera_names(ch, dup, lens, 3) == 0) return 5;
	puts(bh_last_error());
	bh_chimera_close(ch);
	if (bh_chimera_open(argv[1], 0, 0, 16, 3, &ch) == 0) return 6;
	/* a read of 4095 symbols with 254 edits on either side, both strands; then ops that leave the array */
	const uint32_t w[3] = {1, 2, 2}, len[3] = {4095, 4095, 4095};
	const uint32_t ops[6] = {254u << 4 | BHIP_OP_X, 3841u << 4 | BHIP_OP_EQ, 54u << 4 | BHIP_OP_X, 50u << 4 | BHIP_OP_D, 150u << 4 | BHIP_OP_I, 3891u << 4 | BHIP_OP_EQ};
	const BhipChimLine lines[2] = {{0, 1, 0, 2, 0}, {0, 2, 1, 4, 2}};      /* (the second is a reverse line: its edits lie at the read's far end) */
	BhipChimera out[3]; uint64_t info[8];
	if (bh_chimera_host(NULL, 3, w, len, lines, 2, ops, 6, 2, 16, 3, out, info) || out[0].role != 2 || out[0].single != 254) return 7;
	const BhipChimLine bad[1] = {{0, 1, 0, 4, 4}};
	if (bh_chimera_host(NULL, 3, w, len, bad, 1, ops, 6, 2, 16, 3, out, info) != BH_E_USAGE) return 8;
	if (bh_chimera_host(NULL, 0, NULL, NULL, NULL, 0, NULL, 0, 2, 16, 3, NULL, info)) return 10;
	printf("chimera_host_main ok\n");
	return 0;
}
