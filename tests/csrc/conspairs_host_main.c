/* tests/csrc/conspairs_host_main.c -- burst_amd/csrc/host/bh_conspairs.c with bh_consensus.c (the yardstick bh_consensus_pairs_host, the
 * collector, the three files, the life cycle) as a stand-alone program, for a build with -fsanitize=address,undefined
 * (tests/test_conspairs_cpu.py).  TEST INFRASTRUCTURE ONLY.
 *   conspairs_host_main solve IN OUT      IN: u32 n_samples, u32 min_compared, u64 n_segs, u64 n_letters, u64 pair_cap, the segments, the letters;
 *                                         OUT: i64 return code, u64 n_pairs, u64 info[8], the pairs (when the code is 0), then the error text
 *   conspairs_host_main study DIR SAMPLES MIN_BREADTH M    a study through the collector with both plain-C solvers; SAMPLES: a letter per sample,
 *                                         a / b / c = a set of printed lines below, f = a sample that failed alone; the files stay in DIR
 *   conspairs_host_main life DIR          the life cycle and the refusals */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* what the linked files reference and this program never reaches */
int bhip_consensus_run(void *h, const uint8_t *c, const uint64_t *o, uint32_t nq, const BhipPileLine *l, uint64_t nl, const uint32_t *ops, uint64_t no, uint32_t m,
                       BhipConsSeg *s, uint64_t sc, uint64_t *ns, char *le, uint64_t lc, uint64_t *nle, uint64_t info[8]) {
	(void)h; (void)c; (void)o; (void)nq; (void)l; (void)nl; (void)ops; (void)no; (void)m; (void)s; (void)sc; (void)ns; (void)le; (void)lc; (void)nle; (void)info;
	return BHIP_E_DEVICE;
}
int bhip_consensus_pairs(void *h, uint32_t n, const BhipPairSeg *s, uint64_t ns, const char *l, uint64_t nl, uint32_t m, BhipPair *p, uint64_t cap, uint64_t *np, uint64_t info[8]) {
	(void)h; (void)n; (void)s; (void)ns; (void)l; (void)nl; (void)m; (void)p; (void)cap; (void)np; (void)info;
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
/* the records of a traced group, as the report hands them over: 0, 1, 3 plain reads at columns 1, 9, 21; 2 the X read at 21; 4 the D read and
 * 5 the I read at column 1.  A printed line {record, offset, header, unique} lies at position offset + the record's first column */
static const uint64_t rec_idx[6] = {0, 1, 2, 3, 4, 5};
static const BhipPathReq rec_req[6] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {1, 0, 0, 1}, {0, 0, 0, 0}, {2, 0, 0, 1}, {3, 0, 0, 1}};
static const uint32_t rec_first[6] = {1, 9, 21, 21, 1, 1};
static const uint64_t rec_off[7] = {0, 1, 2, 5, 6, 9, 12};
static const uint32_t rec_ops[12] = {W(8, BHIP_OP_EQ), W(8, BHIP_OP_EQ), W(3, BHIP_OP_EQ), W(1, BHIP_OP_X), W(4, BHIP_OP_EQ), W(8, BHIP_OP_EQ),
                                     W(3, BHIP_OP_EQ), W(1, BHIP_OP_D), W(4, BHIP_OP_EQ), W(4, BHIP_OP_EQ), W(1, BHIP_OP_I), W(4, BHIP_OP_EQ)};
/* headers 0 beta (30), 1 alpha x (12), 2 gamma (8); min_depth 2.
 * a: beta 1..8 twice, 9..16 once (N), 21..28 with A at 24 (three reads against one); alpha x 5..12 with column 8 deleted; gamma 1..8
 * b: beta 1..8 twice, 9..16 twice (called), 21..28 plain (T at 24); alpha x 5..12 plain (a base against a's '-'); gamma 1..8
 * c: alpha x 5..12 with the deletion ('-' against '-' with a); beta 21..28 with A at 24; gamma once (a row, no record) */
static BhPathLine set_a[] = {{0, 0, 0, 1}, {0, 0, 0, 1}, {1, 0, 0, 1}, {2, 0, 0, 1}, {2, 0, 0, 1}, {2, 0, 0, 1}, {3, 0, 0, 1}, {4, 4, 1, 1}, {4, 4, 1, 1}, {5, 0, 2, 0}, {5, 0, 2, 0}};
static BhPathLine set_b[] = {{0, 0, 0, 1}, {0, 0, 0, 1}, {0, 8, 0, 1}, {0, 8, 0, 1}, {3, 0, 0, 1}, {3, 0, 0, 1}, {0, 4, 1, 1}, {0, 4, 1, 1}, {0, 0, 2, 1}, {0, 0, 2, 1}};
static BhPathLine set_c[] = {{2, 0, 0, 1}, {2, 0, 0, 1}, {4, 4, 1, 1}, {4, 4, 1, 1}, {0, 0, 2, 1}};

static const char *heads[3] = {"beta", "alpha x", "gamma"};
static const uint32_t lengths[3] = {30, 12, 8};
static BhPileRefs R = {packed, clump_len, 1, 16};

static int exists(const char *path) { FILE *f = fopen(path, "rb"); if (f) fclose(f); return f != NULL; }

static int open_both(const char *prefix, uint32_t min_breadth, uint32_t M, int host_pairs, BhCons **cn, BhConsPairs **cp) {
	if (bh_consensus_open_heads(prefix, 3, heads, lengths, 2, min_breadth, 0, cn)) return 1;
	bh_consensus_set_solver(*cn, bh_consensus_host, &R);
	if (bh_conspairs_open(prefix, M, cp)) return 1;
	if (host_pairs) bh_conspairs_set_solver(*cp, bh_consensus_pairs_host, NULL);
	bh_conspairs_attach(*cp, *cn);
	return 0;
}

static int add_sample(BhCons *cn, char which, const char *out) {
	if (which == 'f') return bh_consensus_sample_failed(cn, out);
	BhPathBuf buf = {set_a, sizeof set_a / sizeof *set_a, sizeof set_a / sizeof *set_a};
	if (which == 'b') { buf.l = set_b; buf.n = buf.cap = sizeof set_b / sizeof *set_b; }
	if (which == 'c') { buf.l = set_c; buf.n = buf.cap = sizeof set_c / sizeof *set_c; }
	const int rc = bh_consensus_collect(cn, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, &buf, 1);
	return rc ? rc : bh_consensus_sample(cn, NULL, out, q_codes, q_off, 4);
}

static int solve(const char *in, const char *out) {
	FILE *f = fopen(in, "rb");
	if (!f) return 2;
	uint32_t n_samples = 0, M = 0; uint64_t ns = 0, nl = 0, cap = 0;
	if (fread(&n_samples, 4, 1, f) != 1 || fread(&M, 4, 1, f) != 1 || fread(&ns, 8, 1, f) != 1 || fread(&nl, 8, 1, f) != 1 || fread(&cap, 8, 1, f) != 1) return 2;
	BhipPairSeg *segs = malloc((size_t)(ns ? ns : 1) * sizeof(*segs));
	char *letters = malloc((size_t)(nl ? nl : 1));
	BhipPair *pairs = malloc((size_t)(cap ? cap : 1) * sizeof(*pairs));
	if (!segs || !letters || !pairs || fread(segs, sizeof(*segs), (size_t)ns, f) != ns || fread(letters, 1, (size_t)nl, f) != nl) return 2;
	fclose(f);
	uint64_t np = 0, info[8];
	const int64_t rc = bh_consensus_pairs_host(NULL, n_samples, ns ? segs : NULL, ns, nl ? letters : NULL, nl, M, cap ? pairs : NULL, cap, &np, info);
	if (!(f = fopen(out, "wb"))) return 2;
	fwrite(&rc, 8, 1, f); fwrite(&np, 8, 1, f); fwrite(info, 8, 8, f);
	if (!rc) fwrite(pairs, sizeof(*pairs), (size_t)np, f);
	if (rc) fputs(bh_last_error(), f);
	fclose(f);
	free(segs); free(letters); free(pairs);
	return 0;
}

int main(int argc, char **argv) {
	if (argc < 3) return 2;
	for (uint32_t c = 0; c < 64; ++c) packed[(c >> 1) * 16] |= (uint8_t)((1 + c % 4) << (4 * (c & 1)));
	if (!strcmp(argv[1], "solve")) return argc < 4 ? 2 : solve(argv[2], argv[3]);
	char *prefix = NULL, *fin[5];
	static const char *const suffix[5] = {"consensus.fa", "consensus.txt", "consensus_pairs.txt", "consensus_identity.txt", "consensus_compared.txt"};
	CHECK(asprintf(&prefix, "%s/P_", argv[2]) > 0);
	for (int k = 0; k < 5; ++k) CHECK(asprintf(&fin[k], "%s%s", prefix, suffix[k]) > 0);
	BhCons *cn = NULL; BhConsPairs *cp = NULL;
	if (!strcmp(argv[1], "study")) {
		if (argc < 6) return 2;
		const char *samples = argv[3];
		CHECK(!open_both(prefix, (uint32_t)atoi(argv[4]), (uint32_t)strtoul(argv[5], NULL, 10), 1, &cn, &cp));
		for (size_t i = 0; samples[i]; ++i) {
			char out[64];
			snprintf(out, sizeof out, "dir/s%d_%c.b6", (int)i, samples[i]);
			CHECK(add_sample(cn, samples[i], out) == BH_OK);
		}
		for (int k = 0; k < 5; ++k) CHECK(!exists(fin[k]));      /* nothing under the final names before the write */
		CHECK(bh_consensus_write(cn) == BH_E_USAGE && strstr(bh_last_error(), "bh_consensus_pairs has not run"));      /* (not final: the pairs come first) */
		CHECK(bh_consensus_pairs(cn, NULL) == BH_OK);
		for (int k = 0; k < 5; ++k) CHECK(!exists(fin[k]));
		CHECK(bh_consensus_pairs(cn, NULL) != BH_OK);      /* once */
		CHECK(bh_consensus_write(cn) == BH_OK);
		bh_conspairs_print_info(cp);
		uint64_t fig[8], us = 1;
		bh_conspairs_last_info(cp, fig, &us);
		printf("figures %lu %lu %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)fig[0], (unsigned long)fig[1], (unsigned long)fig[2], (unsigned long)fig[3], (unsigned long)fig[4],
		       (unsigned long)fig[5], (unsigned long)fig[6], (unsigned long)fig[7], (unsigned long)us);
		bh_consensus_close(cn); bh_conspairs_close(cp);
		for (int k = 0; k < 5; ++k) { CHECK(exists(fin[k])); free(fin[k]); }
		free(prefix);
		puts("conspairs_host_main study ok");
		return 0;
	}
	if (strcmp(argv[1], "life")) return 2;
	/* the option and the names */
	CHECK(bh_conspairs_check_min(0) == BH_E_USAGE && strstr(bh_last_error(), "--consensus-pairs-min") && bh_conspairs_check_min(0x80000000ull) == BH_E_USAGE);
	CHECK(bh_conspairs_check_min(1) == BH_OK && bh_conspairs_check_min(0x7FFFFFFFull) == BH_OK);
	CHECK(bh_conspairs_open(prefix, 0, &cp) == BH_E_USAGE && !cp);
	const char *clash[3] = {"a/s1.b6", "other.b6", "b/s1.txt"}, *fine[2] = {"a/s1.b6", "a/s2.b6"};
	CHECK(bh_conspairs_check_names(clash, 3) == BH_E_USAGE && strstr(bh_last_error(), "'a/s1.b6'") && strstr(bh_last_error(), "'b/s1.txt'") && strstr(bh_last_error(), "--consensus-pairs"));
	CHECK(bh_conspairs_check_names(fine, 2) == BH_OK);
	/* a record covered through position 2^32 - 1: a usage error in the run's terms, final */
	CHECK(bh_conspairs_open(prefix, 1, &cp) == BH_OK);
	const BhipConsSeg last = {0, 0xFFFFFFF0u, 16, 16, 16, 0, 0, 0, 0, 0, 0}, fits = {0, 0xFFFFFFEFu, 16, 16, 16, 0, 0, 0, 0, 0, 0};
	CHECK(bh_conspairs_add(cp, 0, 0, &fits, 1, "ACGTACGTACGTACGT") == BH_OK);
	CHECK(bh_conspairs_add(cp, 1, 0, &last, 1, "ACGTACGTACGTACGT") == BH_E_USAGE && strstr(bh_last_error(), "--consensus-pairs") && strstr(bh_last_error(), "4294967295"));
	CHECK(bh_conspairs_add(cp, 1, 0, &fits, 1, "ACGTACGTACGTACGT") != BH_OK);
	bh_conspairs_close(cp); cp = NULL;
	/* the device solver without a handle: final, no file, no temporary file */
	CHECK(!open_both(prefix, 0, 1, 0, &cn, &cp));
	CHECK(add_sample(cn, 'a', "s1.b6") == BH_OK && add_sample(cn, 'b', "s2.b6") == BH_OK);
	CHECK(bh_consensus_pairs(cn, NULL) == BH_E_DEVICE && strstr(bh_last_error(), "no device handle"));
	CHECK(bh_consensus_write(cn) != BH_OK);
	bh_consensus_close(cn); bh_conspairs_close(cp);
	for (int k = 0; k < 5; ++k) CHECK(!exists(fin[k]));
	/* an abort reaches the collector; a close without a write */
	CHECK(!open_both(prefix, 0, 1, 1, &cn, &cp));
	CHECK(add_sample(cn, 'a', "s1.b6") == BH_OK);
	bh_consensus_abort(cn);
	CHECK(bh_consensus_pairs(cn, NULL) != BH_OK && bh_consensus_write(cn) != BH_OK);
	bh_consensus_close(cn); bh_conspairs_close(cp);
	CHECK(!open_both(prefix, 0, 1, 1, &cn, &cp));
	CHECK(add_sample(cn, 'a', "s1.b6") == BH_OK && bh_consensus_pairs(cn, NULL) == BH_OK);      /* the three temporary files exist now */
	bh_consensus_close(cn); bh_conspairs_close(cp);
	for (int k = 0; k < 5; ++k) CHECK(!exists(fin[k]));
	/* a consensus without a collector is the parent's: no hook is reached */
	CHECK(bh_consensus_open_heads(prefix, 3, heads, lengths, 2, 0, 0, &cn) == BH_OK);
	bh_consensus_set_solver(cn, bh_consensus_host, &R);
	CHECK(bh_consensus_pairs(cn, NULL) == BH_E_USAGE);
	CHECK(add_sample(cn, 'a', "s1.b6") == BH_OK && bh_consensus_write(cn) == BH_OK);
	bh_consensus_close(cn);
	CHECK(exists(fin[0]) && exists(fin[1]) && !exists(fin[2]) && !exists(fin[3]) && !exists(fin[4]));
	CHECK(!remove(fin[0]) && !remove(fin[1]));
	bh_conspairs_close(NULL);
	free(prefix);
	for (int k = 0; k < 5; ++k) free(fin[k]);
	puts("conspairs_host_main life ok");
	return 0;
}
