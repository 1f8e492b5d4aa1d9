/* tests/csrc/taxa_host_main.c -- csrc/host/bh_taxa.c as a stand-alone program (tests/test_taxa_cpu.py builds it with the address and the
 * undefined-behaviour sanitizer): the tree builder on a map file, bh_taxa_host on the hand case of the definition, its refusals, the roll-up,
 * and the table writer with the two as its solvers.  argv[1] = a taxonomy map, argv[2] = prefix of the tables. */
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>

/* no device in this program */
int bhip_taxa_run(void *h, uint32_t nn, const uint32_t *p, uint32_t nh, const uint32_t *hn, uint32_t ng, const uint32_t *gw, const BhipEmLine *l, uint64_t n, uint32_t agree,
                  uint32_t *gn, uint64_t *own, uint64_t *clade, uint64_t info[8]) {
	(void)h; (void)nn; (void)p; (void)nh; (void)hn; (void)ng; (void)gw; (void)l; (void)n; (void)agree; (void)gn; (void)own; (void)clade; (void)info;
	return BHIP_E_DEVICE;
}
int bhip_taxa_rollup(void *h, uint32_t nn, const uint32_t *p, uint32_t nh, const uint32_t *hn, const uint64_t *c, uint64_t *own, uint64_t *clade) {
	(void)h; (void)nn; (void)p; (void)nh; (void)hn; (void)c; (void)own; (void)clade;
	return BHIP_E_DEVICE;
}
const char *bhip_last_error(void) { return "no device in this program"; }

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

int main(int argc, char **argv) {
	if (argc < 3) return 2;
	/* the map of the hand case: a;b;c, a;b;d (with a trailing ';'), a;e, f, none, a;b;c; h6 is not in the map */
	const char *heads[7] = {"h0", "h1", "h2", "h3", "h4", "h5", "h6"};
	BhTax map;
	CHECK(bh_tax_load(argv[1], &map) == BH_OK);
	BhTaxaTree T;
	CHECK(bh_taxa_tree(7, heads, &map, 0, &T) == BH_OK);
	const uint32_t parent[7] = {0, 0, 1, 2, 2, 1, 0}, hnode[7] = {3, 4, 5, 6, 0, 3, 0};
	const char *names[7] = {"Unassigned", "a", "a;b", "a;b;c", "a;b;d", "a;e", "f"};
	CHECK(T.n_nodes == 7 && T.n_headers == 7);
	for (uint32_t v = 0; v < 7 && T.n_nodes == 7; ++v) CHECK(T.parent[v] == parent[v] && !strcmp(T.name[v], names[v]));
	for (uint32_t h = 0; h < 7 && T.n_nodes == 7; ++h) CHECK(T.header_node[h] == hnode[h]);
	bh_taxa_tree_free(&T);
	/* the hand case */
	const uint32_t gw[7] = {3, 1, 1, 1, 1, 1, 9};
	const BhipEmLine ln[13] = {{0, 0}, {1, 0}, {1, 1}, {2, 0}, {2, 5}, {2, 1}, {3, 0}, {3, 2}, {3, 3}, {4, 0}, {4, 4}, {5, 0}, {5, 0}};
	uint32_t gn[7]; uint64_t own[7], clade[7], info[8];
	CHECK(bh_taxa_host(NULL, 7, parent, 7, hnode, 7, gw, ln, 13, 1000, gn, own, clade, info) == BH_OK);
	{ const uint32_t wg[7] = {3, 2, 2, 0, 0, 3, 0xFFFFFFFFu}; const uint64_t wo[7] = {2, 0, 2, 4, 0, 0, 0}, wc[7] = {8, 6, 6, 4, 0, 0, 0}, wi[5] = {12, 6, 8, 2, 3};
	  for (int i = 0; i < 7; ++i) CHECK(gn[i] == wg[i] && own[i] == wo[i] && clade[i] == wc[i]);
	  for (int i = 0; i < 5; ++i) CHECK(info[i] == wi[i]); }
	CHECK(bh_taxa_host(NULL, 7, parent, 7, hnode, 7, gw, ln, 13, 600, gn, own, clade, info) == BH_OK);
	{ const uint32_t wg[7] = {3, 2, 3, 1, 0, 3, 0xFFFFFFFFu}; const uint64_t wo[7] = {1, 1, 1, 5, 0, 0, 0}, wc[7] = {8, 7, 6, 5, 0, 0, 0}, wi[5] = {12, 6, 8, 1, 3};
	  for (int i = 0; i < 7; ++i) CHECK(gn[i] == wg[i] && own[i] == wo[i] && clade[i] == wc[i]);
	  for (int i = 0; i < 5; ++i) CHECK(info[i] == wi[i]); }
	CHECK(bh_taxa_host(NULL, 7, parent, 7, hnode, 7, gw, ln, 0, 1000, gn, own, clade, info) == BH_OK && gn[0] == 0xFFFFFFFFu && !clade[0] && !info[0]);
	/* refusals */
	{
		const uint32_t p_root[2] = {1, 0}, p_self[3] = {0, 0, 2}, p_order[4] = {0, 0, 0, 1}, hbad[1] = {7};
		const BhipEmLine badg[1] = {{7, 0}}, badr[1] = {{0, 7}};
		CHECK(bh_taxa_host(NULL, 2, p_root, 7, hnode, 7, gw, ln, 13, 1000, gn, own, clade, info) == BH_E_USAGE);
		CHECK(bh_taxa_host(NULL, 3, p_self, 0, NULL, 7, gw, ln, 0, 1000, gn, own, clade, info) == BH_E_USAGE);
		CHECK(bh_taxa_host(NULL, 4, p_order, 0, NULL, 7, gw, ln, 0, 1000, gn, own, clade, info) == BH_E_USAGE);
		CHECK(bh_taxa_host(NULL, 7, parent, 1, hbad, 7, gw, ln, 0, 1000, gn, own, clade, info) == BH_E_USAGE);
		CHECK(bh_taxa_host(NULL, 7, parent, 7, hnode, 7, gw, badg, 1, 1000, gn, own, clade, info) == BH_E_USAGE);
		CHECK(bh_taxa_host(NULL, 7, parent, 7, hnode, 7, gw, badr, 1, 1000, gn, own, clade, info) == BH_E_USAGE);
		CHECK(bh_taxa_host(NULL, 7, parent, 7, hnode, 7, gw, ln, 13, 500, gn, own, clade, info) == BH_E_USAGE);
		CHECK(bh_taxa_host(NULL, 7, parent, 7, hnode, 7, gw, ln, 13, 1001, gn, own, clade, info) == BH_E_USAGE);
		CHECK(bh_taxa_host(NULL, 7, parent, 7, hnode, 7, gw, ln, (uint64_t)1 << 31, 1000, gn, own, clade, info) == BH_E_USAGE);
		uint32_t chain[66]; uint64_t o66[66], c66[66];
		for (uint32_t v = 0; v < 66; ++v) chain[v] = v ? v - 1 : 0;
		CHECK(bh_taxa_host(NULL, 65, chain, 0, NULL, 0, NULL, NULL, 0, 1000, NULL, o66, c66, info) == BH_OK);      /* 64 levels */
		CHECK(bh_taxa_host(NULL, 66, chain, 0, NULL, 0, NULL, NULL, 0, 1000, NULL, o66, c66, info) == BH_E_USAGE);
		CHECK(bh_taxa_check_opts(NULL, 0, 1000) == BH_E_USAGE && bh_taxa_check_opts("m", 1, 500) == BH_E_USAGE && bh_taxa_check_opts("m", 1, 501) == BH_OK);
	}
	/* the roll-up */
	{
		const uint64_t cnt[7] = {5, 7, 11, 13, 17, (uint64_t)1 << 62, 0};
		CHECK(bh_taxa_rollup_host(NULL, 7, parent, 7, hnode, cnt, own, clade) == BH_OK);
		CHECK(own[0] == 17 && own[3] == ((uint64_t)1 << 62) + 5 && own[4] == 7 && own[5] == 11 && own[6] == 13 && !own[1] && !own[2]);
		CHECK(clade[0] == ((uint64_t)1 << 62) + 53 && clade[1] == ((uint64_t)1 << 62) + 23 && clade[2] == ((uint64_t)1 << 62) + 12);
	}
	/* the tables: two samples and a failed one between them, the plain-C definitions as the solvers, abundance counts for the first */
	{
		BhTaxa *tx = NULL;
		CHECK(bh_taxa_open_heads(argv[2], 7, heads, &map, 0, 1000, &tx) == BH_OK);
		bh_taxa_set_solver(tx, bh_taxa_host, bh_taxa_rollup_host, NULL);
		const uint32_t uq[13] = {0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 5, 5};
		BhipCovLine pl[13];
		for (int i = 0; i < 13; ++i) { pl[i].ref = ln[i].ref; pl[i].st = 1; pl[i].ed = 2; pl[i].w = gw[uq[i]]; }
		const uint64_t em[7] = {(uint64_t)3 << 30, (uint64_t)1 << 29, 0, 0, (uint64_t)1 << 30, 0, 0};
		CHECK(bh_taxa_sample(tx, NULL, "dir/one.b6", uq, pl, 13, em) == BH_OK);
		CHECK(bh_taxa_sample_failed(tx, "dir/two.b6") == BH_OK);
		pl[0].w = 2 | 0x80000000u;
		CHECK(bh_taxa_sample(tx, NULL, "three", uq, pl, 1, NULL) == BH_OK);
		uint32_t nc = 0, nn = 0, nl = 0, nel = 0;
		bh_taxa_dims(tx, &nc, &nn);
		CHECK(nc == 4 && nn == 7);
		uint64_t cols[4 * 4 * 7];
		CHECK(bh_taxa_stats(tx, cols) == BH_OK);
		CHECK(cols[0] == 2 && cols[3] == 6 && cols[7 + 3] == 4 && cols[14 + 3] == 0 && cols[21 + 3] == 2);      /* own: Dataset, one, two, three */
		CHECK(cols[28 + 0] == 10 && cols[28 + 7 + 1] == 6);                                                      /* clade */
		CHECK(bh_taxa_write(tx, &nl, &nel) == BH_OK && nl == 3 && nel == 3);
		bh_taxa_close(tx);
	}
	bh_tax_free(&map);
	if (fails) return 1;
	puts("taxa_host_main ok");
	return 0;
}
