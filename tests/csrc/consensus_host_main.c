/* tests/csrc/consensus_host_main.c -- burst_amd/csrc/host/bh_consensus.c (the yardstick bh_consensus_host, the collector, the two files, the
 * life cycle) as a stand-alone program on hand-made inputs, for a build with -fsanitize=address,undefined (tests/test_consensus_cpu.py).
 * TEST INFRASTRUCTURE ONLY.  usage: consensus_host_main DIR */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* what bh_consensus.c references and this program never reaches */
int bhip_consensus_run(void *h, const uint8_t *c, const uint64_t *o, uint32_t nq, const BhipPileLine *l, uint64_t nl, const uint32_t *ops, uint64_t no, uint32_t m,
                       BhipConsSeg *s, uint64_t sc, uint64_t *ns, char *le, uint64_t lc, uint64_t *nle, uint64_t info[8]) {
	(void)h; (void)c; (void)o; (void)nq; (void)l; (void)nl; (void)ops; (void)no; (void)m; (void)s; (void)sc; (void)ns; (void)le; (void)lc; (void)nle; (void)info;
	return BHIP_E_DEVICE;
}
const char *bhip_last_error(void) { return "no device in this program"; }
int bh_cov_read_lengths(const char *file, const char *flag, uint32_t n, const char *const *heads, uint32_t *len) { (void)file; (void)flag; (void)n; (void)heads; (void)len; return BH_E_IO; }
int bh_cov_default_lengths(const BhDb *db, void *hh, uint32_t *len) { (void)db; (void)hh; (void)len; return BH_E_DEVICE; }
int bh_paths_add_collector(BhPaths *p, bh_paths_collect_text_fn fn, void *ctx, int columns) { (void)p; (void)fn; (void)ctx; (void)columns; return BH_OK; }

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s [%s]\n", __LINE__, #c, bh_last_error()); return 1; } } while (0)
#define W(n, code) ((uint32_t)(n) << 4 | (code))

/* one clump of 16 lanes, 64 columns; lane 0 = ACGT ACGT ... (codes 1 2 3 4), the other lanes empty */
static uint8_t packed[32 * 16];
static const uint32_t clump_len[1] = {64};
/* query entries: 0 ACGTACGT, 1 ACGAACGT (X in the fourth symbol), 2 ACG ACGT (a column deleted), 3 ACGT G ACGT (a symbol inserted) */
static const uint8_t q_codes[] = {1, 2, 3, 4, 1, 2, 3, 4,  1, 2, 3, 1, 1, 2, 3, 4,  1, 2, 3, 1, 2, 3, 4,  1, 2, 3, 4, 3, 1, 2, 3, 4};
static const uint64_t q_off[] = {0, 8, 16, 23, 32};
static const uint32_t all_ops[] = {W(8, BHIP_OP_EQ), W(3, BHIP_OP_EQ), W(1, BHIP_OP_X), W(4, BHIP_OP_EQ), W(3, BHIP_OP_EQ), W(1, BHIP_OP_D), W(4, BHIP_OP_EQ),
                                   W(4, BHIP_OP_EQ), W(1, BHIP_OP_I), W(4, BHIP_OP_EQ)};

static char *slurp(const char *path) {
	FILE *f = fopen(path, "rb");
	if (!f) return NULL;
	char *s = calloc(1, 1 << 16);
	if (s) (void)fread(s, 1, (1 << 16) - 1, f);
	fclose(f);
	return s;
}

static int seg_is(const BhipConsSeg *g, uint32_t header, uint32_t pos, uint32_t len, uint32_t called, uint32_t same, uint32_t subst, uint32_t del, uint32_t ins_major, uint64_t off) {
	return g->header == header && g->pos == pos && g->len == len && g->called == called && g->same == same && g->subst == subst && g->del == del && g->ambig == 0 &&
	       g->ins_major == ins_major && g->pad == 0 && g->off == off;
}

/* the records of a traced group, as the report hands them over */
static const uint64_t rec_idx[6] = {0, 1, 2, 3, 4, 5};
static const BhipPathReq rec_req[6] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {1, 0, 0, 1}, {0, 0, 0, 0}, {2, 0, 0, 1}, {3, 0, 0, 1}};
static const uint32_t rec_first[6] = {1, 9, 21, 21, 1, 1};
static const uint64_t rec_off[7] = {0, 1, 2, 5, 6, 9, 12};
static const uint32_t rec_ops[12] = {W(8, BHIP_OP_EQ), W(8, BHIP_OP_EQ), W(3, BHIP_OP_EQ), W(1, BHIP_OP_X), W(4, BHIP_OP_EQ), W(8, BHIP_OP_EQ),
                                     W(3, BHIP_OP_EQ), W(1, BHIP_OP_D), W(4, BHIP_OP_EQ), W(4, BHIP_OP_EQ), W(1, BHIP_OP_I), W(4, BHIP_OP_EQ)};

int main(int argc, char **argv) {
	if (argc < 2) return 2;
	for (uint32_t c = 0; c < 64; ++c) packed[(c >> 1) * 16] |= (uint8_t)((1 + c % 4) << (4 * (c & 1)));
	BhPileRefs R = {packed, clump_len, 1, 16};
	/* ---- the yardstick: header 0: 1..8 twice, 9..16 once, 21..28 with three reads that show A at 24 and one that shows T; header 1: a
	 * deletion at 8 in both reads; header 2: both reads insert behind 4 ---- */
	const BhipPileLine lines[6] = {{0, 0, 1, 0, 1, 2, 1, 0}, {0, 0, 9, 0, 9, 1, 1, 0}, {1, 0, 21, 0, 21, 3, 3, 1}, {0, 0, 21, 0, 21, 1, 1, 0},
	                               {2, 0, 1, 1, 5, 2, 3, 4}, {3, 0, 1, 2, 1, 2, 3, 7}};
	BhipConsSeg segs[8]; char letters[64]; uint64_t ns = 0, nl = 0, info[8];
	CHECK(bh_consensus_host(&R, q_codes, q_off, 4, lines, 6, all_ops, 10, 2, segs, 8, &ns, letters, 64, &nl, info) == BH_OK);
	CHECK(ns == 4 && nl == 40 && info[2] == 4 && info[3] == 40);
	CHECK(info[0] == 3 && info[1] == 3);      /* events: the X, the D and the mark of one line each, whatever its weight */
	CHECK(seg_is(&segs[0], 0, 1, 16, 8, 8, 0, 0, 0, 0) && !memcmp(letters, "ACGTACGTNNNNNNNN", 16));
	CHECK(seg_is(&segs[1], 0, 21, 8, 8, 7, 1, 0, 0, 16) && !memcmp(letters + 16, "ACGAACGT", 8));
	CHECK(seg_is(&segs[2], 1, 5, 8, 8, 7, 0, 1, 0, 24) && !memcmp(letters + 24, "ACG-ACGT", 8));
	CHECK(seg_is(&segs[3], 2, 1, 8, 8, 8, 0, 0, 1, 32) && !memcmp(letters + 32, "ACGTACGT", 8));
	/* a gap of one position makes two segments; min_depth above every depth calls nothing */
	const BhipPileLine gap[2] = {{0, 0, 1, 0, 1, 1, 1, 0}, {0, 0, 9, 0, 10, 1, 1, 0}};
	CHECK(bh_consensus_host(&R, q_codes, q_off, 4, gap, 2, all_ops, 10, 1000, segs, 8, &ns, letters, 64, &nl, info) == BH_OK);
	CHECK(ns == 2 && nl == 16 && segs[0].len == 8 && segs[1].pos == 10 && segs[1].off == 8 && !segs[0].called && !segs[1].called && !memcmp(letters, "NNNNNNNNNNNNNNNN", 16));
	/* both capacities: the counts come back, nothing is written */
	memset(letters, '#', sizeof letters);
	CHECK(bh_consensus_host(&R, q_codes, q_off, 4, lines, 6, all_ops, 10, 2, segs, 3, &ns, letters, 64, &nl, info) == BH_E_CAPACITY && ns == 4 && nl == 40 && letters[0] == '#');
	CHECK(bh_consensus_host(&R, q_codes, q_off, 4, lines, 6, all_ops, 10, 2, segs, 8, &ns, letters, 39, &nl, info) == BH_E_CAPACITY && ns == 4 && nl == 40 && letters[0] == '#');
	CHECK(bh_consensus_host(&R, q_codes, q_off, 4, lines, 0, all_ops, 10, 2, segs, 8, &ns, letters, 64, &nl, info) == BH_OK && ns == 0 && nl == 0);
	/* arguments */
	CHECK(bh_consensus_host(&R, q_codes, q_off, 4, lines, 6, all_ops, 10, 0, segs, 8, &ns, letters, 64, &nl, info) == BH_E_USAGE && strstr(bh_last_error(), "min_depth"));
	BhipPileLine bad = lines[0];
	bad.pos = 0;
	CHECK(bh_consensus_host(&R, q_codes, q_off, 4, &bad, 1, all_ops, 10, 1, segs, 8, &ns, letters, 64, &nl, info) == BH_E_USAGE && strstr(bh_last_error(), "line 0"));
	bad = lines[0]; bad.ref_first = 60;
	CHECK(bh_consensus_host(&R, q_codes, q_off, 4, &bad, 1, all_ops, 10, 1, segs, 8, &ns, letters, 64, &nl, info) == BH_E_USAGE && strstr(bh_last_error(), "leave a clump"));

	/* ---- the object: headers 0 beta, 1 alpha x, 2 gamma (strcmp order: alpha x, beta, gamma) ---- */
	char *prefix = NULL, *fa = NULL, *tx = NULL;
	CHECK(asprintf(&prefix, "%s/P_", argv[1]) > 0 && asprintf(&fa, "%sconsensus.fa", prefix) > 0 && asprintf(&tx, "%sconsensus.txt", prefix) > 0);
	const char *heads[3] = {"beta", "alpha x", "gamma"};
	uint32_t lengths[3] = {30, 12, 8};
	BhCons *cn = NULL;
	CHECK(bh_consensus_open_heads(prefix, 3, heads, lengths, 0, 0, 0, &cn) == BH_E_USAGE && !cn && strstr(bh_last_error(), "--consensus-min-depth"));
	CHECK(bh_consensus_open_heads(prefix, 3, heads, lengths, 2, 1001, 0, &cn) == BH_E_USAGE && !cn && strstr(bh_last_error(), "--consensus-min-breadth"));
	CHECK(bh_consensus_open_heads(prefix, 3, heads, lengths, 2, 0, 0, &cn) == BH_OK && cn);
	bh_consensus_set_solver(cn, bh_consensus_host, &R);
	/* the printed lines: a duplicate read prints its record's line again, right behind it */
	BhPathLine n1[] = {{0, 0, 0, 1}, {0, 0, 0, 1}, {1, 0, 0, 1}, {2, 0, 0, 1}, {2, 0, 0, 1}, {2, 0, 0, 1}, {3, 0, 0, 1}};
	BhPathLine n2[] = {{4, 4, 1, 1}, {4, 4, 1, 1}, {5, 0, 2, 0}, {5, 0, 2, 0}};
	BhPathBuf bufs[2] = {{n1, 7, 7}, {n2, 4, 4}};
	CHECK(bh_consensus_collect(cn, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, bufs, 2) == BH_OK);
	CHECK(bh_consensus_sample(cn, NULL, "dir/s1.b6", q_codes, q_off, 4) == BH_OK);
	bh_consensus_print_info(cn);
	CHECK(bh_consensus_collect(cn, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, bufs, 2) == BH_OK);
	CHECK(bh_consensus_sample_failed(cn, "broken.b6") == BH_OK);      /* its lines are dropped */
	BhPathLine n3[] = {{5, 0, 2, 1}};
	BhPathBuf one = {n3, 1, 1};
	CHECK(bh_consensus_collect(cn, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, &one, 1) == BH_OK);
	CHECK(bh_consensus_sample(cn, NULL, "s2.b6", q_codes, q_off, 4) == BH_OK);      /* depth 1 under min_depth 2: a row, no record */
	BhConsRow rows[8];
	CHECK(bh_consensus_rows(cn, rows, 8) == 4 && rows[0].header == 1 && rows[0].sample == 0 && rows[1].header == 0 && rows[3].sample == 2 && rows[3].record == 0);
	CHECK(!slurp(fa) && !slurp(tx));      /* nothing under the final names before the write */
	CHECK(bh_consensus_write(cn) == BH_OK);
	bh_consensus_close(cn);
	char *got_fa = slurp(fa), *got_tx = slurp(tx);
	CHECK(got_fa && got_tx);
	CHECK(!strcmp(got_fa, ">s1|alpha x\nNNNNACG-ACGT\n>s1|beta\nACGTACGTNNNNNNNNNNNNACGAACGTNN\n>s1|gamma\nACGTACGT\n"));
	CHECK(!strcmp(got_tx, "#Reference\tSample\tLength\tCovered\tCalled\tSame\tSubst\tDel\tAmbig\tInsMajor\tRecord\n"
	                      "alpha x\ts1\t12\t8\t8\t7\t0\t1\t0\t0\t1\nbeta\ts1\t30\t24\t16\t15\t1\t0\t0\t0\t1\ngamma\ts1\t8\t8\t8\t8\t0\t0\t0\t1\t1\n"
	                      "gamma\ts2\t8\t8\t0\t0\t0\t0\t0\t0\t0\n"));
	free(got_fa); free(got_tx);
	CHECK(!remove(fa) && !remove(tx));
	/* unique reads only: the two lines on gamma are not unique; min_breadth 1000 of beta's 30 positions is not reached */
	CHECK(bh_consensus_open_heads(prefix, 3, heads, lengths, 2, 1000, 1, &cn) == BH_OK);
	bh_consensus_set_solver(cn, bh_consensus_host, &R);
	CHECK(bh_consensus_collect(cn, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, bufs, 2) == BH_OK);
	CHECK(bh_consensus_sample(cn, NULL, "u.b6", q_codes, q_off, 4) == BH_OK && bh_consensus_write(cn) == BH_OK);
	bh_consensus_close(cn);
	got_fa = slurp(fa); got_tx = slurp(tx);
	CHECK(got_fa && got_tx && !strcmp(got_fa, "") && strstr(got_tx, "alpha x\tu\t12\t8\t8\t7\t0\t1\t0\t0\t0\nbeta\tu\t30\t24\t16\t15\t1\t0\t0\t0\t0\n") && !strstr(got_tx, "gamma"));
	free(got_fa); free(got_tx);
	CHECK(!remove(fa) && !remove(tx));
	/* a placement beyond the length of its header: a usage error that names it, and no file */
	lengths[2] = 7;
	CHECK(bh_consensus_open_heads(prefix, 3, heads, lengths, 2, 0, 0, &cn) == BH_OK);
	bh_consensus_set_solver(cn, bh_consensus_host, &R);
	CHECK(bh_consensus_collect(cn, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, bufs, 2) == BH_OK);
	CHECK(bh_consensus_sample(cn, NULL, "s1.b6", q_codes, q_off, 4) == BH_E_USAGE && strstr(bh_last_error(), "'gamma'") && strstr(bh_last_error(), "--consensus"));
	puts(bh_last_error());
	CHECK(bh_consensus_write(cn) != BH_OK && bh_consensus_collect(cn, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, bufs, 2) != BH_OK);
	bh_consensus_close(cn);
	CHECK(!slurp(fa) && !slurp(tx));
	/* an abort, a close without a write, the device solver without a handle */
	lengths[2] = 8;
	CHECK(bh_consensus_open_heads(prefix, 3, heads, lengths, 2, 0, 0, &cn) == BH_OK);
	CHECK(bh_consensus_collect(cn, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, bufs, 2) == BH_OK);
	CHECK(bh_consensus_sample(cn, NULL, "s1.b6", q_codes, q_off, 4) == BH_E_DEVICE && strstr(bh_last_error(), "no device handle"));
	bh_consensus_close(cn);
	CHECK(bh_consensus_open_heads(prefix, 3, heads, lengths, 2, 0, 0, &cn) == BH_OK);
	bh_consensus_abort(cn);
	CHECK(bh_consensus_write(cn) != BH_OK);
	bh_consensus_close(cn);
	CHECK(!slurp(fa) && !slurp(tx));
	free(prefix); free(fa); free(tx);
	puts("consensus_host_main ok");
	return 0;
}
