/* tests/csrc/em_host_main.c -- csrc/host/bh_em.c as a stand-alone program (tests/test_abundance_cpu.py builds it with the address and the
 * undefined-behaviour sanitizer): bh_em_host on the hand cases of the definition, its refusals, and the table writer with bh_em_host as the
 * solver.  argv[1] = prefix of the table. */
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>

/* no device in this program */
int bhip_em_run(void *h, uint32_t nh, uint32_t ng, const uint32_t *gw, const BhipEmLine *l, uint64_t n, uint32_t it, uint64_t tol, uint64_t *c, uint64_t info[8]) {
	(void)h; (void)nh; (void)ng; (void)gw; (void)l; (void)n; (void)it; (void)tol; (void)c; (void)info;
	return BHIP_E_DEVICE;
}
const char *bhip_last_error(void) { return "no device in this program"; }

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

static void run(uint32_t nh, uint32_t ng, const uint32_t *gw, const BhipEmLine *l, uint64_t n, uint32_t iters, uint64_t tol, const uint64_t *want, const uint64_t *info5) {
	uint64_t c[8] = {0}, info[8];
	CHECK(bh_em_host(NULL, nh, ng, gw, l, n, iters, tol, c, info) == BH_OK);
	for (uint32_t h = 0; h < nh; ++h) CHECK(c[h] == want[h]);
	for (int k = 0; k < 5; ++k) CHECK(info[k] == info5[k]);
}

int main(int argc, char **argv) {
	if (argc < 2) return 2;
	/* case 1: headers A, B, C; three reads on {A}, one on {B}, four on {A, B}, the last with its A line twice */
	const uint32_t w8[8] = {1, 1, 1, 1, 1, 1, 1, 1};
	const BhipEmLine c1[13] = {{0, 0}, {1, 0}, {2, 0}, {3, 1}, {4, 0}, {4, 1}, {5, 1}, {5, 0}, {6, 0}, {6, 1}, {7, 0}, {7, 1}, {7, 0}};
	{ const uint64_t want[3] = {5368709120ull, 3221225472ull, 0}, info[5] = {1, 12, 3, 4294967296ull, 0}; run(3, 8, w8, c1, 13, 1, 0, want, info); }
	{ const uint64_t want[3] = {5905580032ull, 2684354560ull, 0}, info[5] = {2, 12, 3, 536870912ull, 0}; run(3, 8, w8, c1, 13, 2, 0, want, info); }
	{ const uint64_t want[3] = {6174015488ull, 2415919104ull, 0}, info[5] = {3, 12, 3, 268435456ull, 0}; run(3, 8, w8, c1, 13, 3, 0, want, info); }
	{ const uint64_t want[3] = {6442449920ull, 2147484672ull, 0}, info[5] = {21, 12, 3, 1024, 1}; run(3, 8, w8, c1, 13, 1000, 1024, want, info); }
	{ const uint64_t want[3] = {6442450944ull, 2147483648ull, 0}, info[5] = {31, 12, 3, 0, 1}; run(3, 8, w8, c1, 13, 1000, 0, want, info); }
	/* cases 2, 3, 4 */
	{ const uint32_t w[1] = {1}; const BhipEmLine l[3] = {{0, 0}, {0, 1}, {0, 2}};
	  const uint64_t want[3] = {357913942, 357913941, 357913941}, info[5] = {2, 3, 1, 0, 1}; run(3, 1, w, l, 3, 1000, 1024, want, info); }
	{ const uint32_t w[1] = {5}; const BhipEmLine l[3] = {{0, 1}, {0, 2}, {0, 3}};
	  const uint64_t want[4] = {0, 1789569710, 1789569705, 1789569705}, info[5] = {2, 3, 1, 0, 1}; run(4, 1, w, l, 3, 1000, 1024, want, info); }
	{ const uint32_t w[2] = {1, 1}; const BhipEmLine l[2] = {{0, 0}, {1, 1}};
	  const uint64_t want[2] = {1073741824, 1073741824}, info[5] = {1, 2, 2, 0, 1}; run(2, 2, w, l, 2, 1000, 1024, want, info); }
	/* nothing takes part: no line, or only groups without reads */
	{ const uint32_t w[2] = {0, 0}; const BhipEmLine l[2] = {{0, 0}, {1, 1}};
	  const uint64_t want[2] = {0, 0}, info[5] = {0, 0, 0, 0, 0}; run(2, 2, w, l, 2, 10, 0, want, info); run(2, 2, w, l, 0, 10, 0, want, info); }
	/* refusals */
	{
		uint64_t c[4], info[8];
		const uint32_t big[2] = {0x7FFFFFFFu, 1};
		const BhipEmLine l[2] = {{0, 0}, {1, 1}}, badg[1] = {{2, 0}}, badr[1] = {{0, 3}};
		CHECK(bh_em_host(NULL, 3, 2, big, l, 2, 10, 0, c, info) == BH_E_USAGE);
		CHECK(bh_em_host(NULL, 3, 2, w8, badg, 1, 10, 0, c, info) == BH_E_USAGE);
		CHECK(bh_em_host(NULL, 3, 2, w8, badr, 1, 10, 0, c, info) == BH_E_USAGE);
		CHECK(bh_em_host(NULL, 3, 2, w8, l, 2, 0, 0, c, info) == BH_E_USAGE);
		CHECK(bh_em_host(NULL, 3, 2, w8, l, (uint64_t)1 << 31, 10, 0, c, info) == BH_E_USAGE);
		CHECK(bh_em_host(NULL, 3, 2, w8, l, 2, 10, 0, c, info) == BH_OK && c[0] == 1073741824 && c[1] == 1073741824 && c[2] == 0);
	}
	/* the table: two samples and a failed one between them, bh_em_host as the solver */
	{
		const char *heads[3] = {"zeta", "alpha", "mid"};
		BhEm *em = NULL;
		CHECK(bh_em_open_heads(argv[1], 3, heads, 1000, 0, &em) == BH_OK);
		bh_em_set_solver(em, bh_em_host, NULL);
		const uint32_t uq[13] = {0, 1, 2, 3, 4, 4, 5, 5, 6, 6, 7, 7, 7};
		BhipCovLine pl[13];
		for (int i = 0; i < 13; ++i) { pl[i].ref = c1[i].ref; pl[i].st = 1; pl[i].ed = 2; pl[i].w = 1; }
		CHECK(bh_em_sample(em, NULL, "dir/one.b6", uq, pl, 13) == BH_OK);
		CHECK(bh_em_sample_failed(em, "dir/two.b6") == BH_OK);
		pl[0].w = 3 | 0x80000000u;
		CHECK(bh_em_sample(em, NULL, "three", uq, pl, 1) == BH_OK);
		uint64_t cols[4 * 3];
		CHECK(bh_em_stats(em, cols) == BH_OK);
		CHECK(cols[3] == 6442450944ull && cols[4] == 2147483648ull && cols[5] == 0 && cols[6] == 0 && cols[7] == 0 && cols[9] == 3221225472ull);
		CHECK(cols[0] == cols[3] + cols[9] && cols[1] == cols[4] && cols[2] == 0);
		CHECK(bh_em_write(em) == BH_OK);
		bh_em_close(em);
	}
	if (fails) return 1;
	puts("em_host_main ok");
	return 0;
}
