/* tests/csrc/vcfstudy_host_main.c -- burst_amd/csrc/host/bh_vcfstudy.c with bh_vcf.c (the yardstick bh_site_counts_host, the collector, the
 * writer of PREFIXstudy.vcf, the life cycle) as a stand-alone program on hand-made inputs, for a build with -fsanitize=address,undefined
 * (tests/test_vcfstudy_cpu.py).  TEST INFRASTRUCTURE ONLY.  usage: vcfstudy_host_main DIR */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* what the linked files reference and this program never reaches */
int bhip_pile_run(void *h, const uint8_t *c, const uint64_t *o, uint32_t nq, const BhipPileLine *l, uint64_t nl, const uint32_t *ops, uint64_t no, uint32_t d, uint32_t a,
                  BhipPileSite *s, uint64_t cap, uint64_t *ns, uint64_t info[8]) {
	(void)h; (void)c; (void)o; (void)nq; (void)l; (void)nl; (void)ops; (void)no; (void)d; (void)a; (void)s; (void)cap; (void)ns; (void)info;
	return BHIP_E_DEVICE;
}
int bhip_alleles_run(void *h, const uint8_t *c, const uint64_t *o, uint32_t nq, const BhipPileLine *l, uint64_t nl, const uint32_t *ops, uint64_t no, uint32_t d, uint32_t a,
                     BhipAllele *al, uint64_t cap, uint64_t *na, uint8_t *codes, uint64_t cc, uint64_t *nc, uint64_t info[8]) {
	(void)h; (void)c; (void)o; (void)nq; (void)l; (void)nl; (void)ops; (void)no; (void)d; (void)a; (void)al; (void)cap; (void)na; (void)codes; (void)cc; (void)nc; (void)info;
	return BHIP_E_DEVICE;
}
int bhip_site_counts(void *h, const BhipCountRange *r, uint64_t nr, const BhipPileSite *s, uint64_t ns, const BhipAllele *a, uint64_t na, const BhipCountRecord *q, uint64_t nq,
                     BhipCountCell *cells, uint64_t info[8]) {
	(void)h; (void)r; (void)nr; (void)s; (void)ns; (void)a; (void)na; (void)q; (void)nq; (void)cells; (void)info;
	return BHIP_E_DEVICE;
}
int bhip_md_tags(void *h, const BhipPathReq *r, const uint32_t *f, const uint64_t *off, const uint32_t *ops, uint64_t n, char *md, uint64_t cap, uint64_t *md_off, uint32_t *nm, uint64_t info[8]) {
	(void)h; (void)r; (void)f; (void)off; (void)ops; (void)n; (void)md; (void)cap; (void)md_off; (void)nm; (void)info;
	return BHIP_E_DEVICE;
}
const char *bhip_last_error(void) { return "no device in this program"; }
int bh_cov_read_lengths(const char *file, const char *flag, uint32_t n, const char *const *heads, uint32_t *len) { (void)file; (void)flag; (void)n; (void)heads; (void)len; return BH_E_IO; }
int bh_cov_default_lengths(const BhDb *db, void *hh, uint32_t *len) { (void)db; (void)hh; (void)len; return BH_E_DEVICE; }
void bh_paths_set_collector(BhPaths *p, bh_paths_collect_fn fn, void *ctx, int columns) { (void)p; (void)fn; (void)ctx; (void)columns; }
size_t bh_cigar_text(const uint32_t *ops, uint64_t n, char *out, size_t cap) { (void)ops; (void)n; (void)out; (void)cap; return 0; }
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
 * 5 the I read at column 1 */
static const uint64_t rec_idx[6] = {0, 1, 2, 3, 4, 5};
static const BhipPathReq rec_req[6] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {1, 0, 0, 1}, {0, 0, 0, 0}, {2, 0, 0, 1}, {3, 0, 0, 1}};
static const uint32_t rec_first[6] = {1, 9, 21, 21, 1, 1};
static const uint64_t rec_off[7] = {0, 1, 2, 5, 6, 9, 12};
static const uint32_t rec_ops[12] = {W(8, BHIP_OP_EQ), W(8, BHIP_OP_EQ), W(3, BHIP_OP_EQ), W(1, BHIP_OP_X), W(4, BHIP_OP_EQ), W(8, BHIP_OP_EQ),
                                     W(3, BHIP_OP_EQ), W(1, BHIP_OP_D), W(4, BHIP_OP_EQ), W(4, BHIP_OP_EQ), W(1, BHIP_OP_I), W(4, BHIP_OP_EQ)};

static char *slurp(const char *path) {
	FILE *f = fopen(path, "rb");
	if (!f) return NULL;
	char *s = calloc(1, 1 << 16);
	if (s && !fread(s, 1, (1 << 16) - 1, f)) s[0] = 0;
	fclose(f);
	return s;
}
static int cell_is(const BhipCountCell *c, uint32_t depth, uint32_t a, uint32_t cc, uint32_t g, uint32_t t, uint32_t count) {
	return c->depth == depth && c->n[0] == a && c->n[1] == cc && c->n[2] == g && c->n[3] == t && c->count == count;
}

static BhVcf *open_vcf(const BhPileRefs *R, BhVcfStudy *st) {
	static const char *heads[3] = {"beta", "alpha x", "gamma"};
	static const uint32_t lengths[3] = {30, 12, 8};
	BhVcf *v = NULL;
	if (bh_vcf_open_heads(3, heads, lengths, 2, 2, 0, &v)) return NULL;
	bh_vcf_set_solver(v, bh_pile_host, (void *)R, bh_alleles_host, (void *)R);
	bh_vcf_set_study(v, st);
	return v;
}

int main(int argc, char **argv) {
	if (argc < 2) return 2;
	for (uint32_t c = 0; c < 64; ++c) packed[(c >> 1) * 16] |= (uint8_t)((1 + c % 4) << (4 * (c & 1)));
	BhPileRefs R = {packed, clump_len, 1, 16};
	/* ---- the yardstick ---- */
	const BhipCountRange ranges[5] = {{3, 10, 11, 2}, {4, 1, 5, 7}, {3, 15, 0, 5}, {3, 12, 3, 4}, {5, 0xFFFFFFFFu - 100, 100, 3}};
	const BhipPileSite sites[1] = {{3, 12, 2, 6, {1, 5, 0, 0, 0, 0}, 0}};
	const BhipAllele alleles[2] = {{3, 14, 2, 1, 6, 1, 0, 0}, {3, 14, 2ull << 60 | 1ull << 56 | 2ull << 52, 1, 6, 2, 0, 0}};
	const BhipCountRecord recs[8] = {{3, 20, 0, 4, 0}, {4, 1, 0, 1, 0}, {3, 21, 0, 1, 0}, {3, 15, 0, 3, 0}, {3, 12, 0, 2, 0}, {5, 0xFFFFFFFEu, 0, 1, 0},
	                                 {3, 14, 2, 0, 0}, {3, 14, 3, 0, 0}};
	BhipCountCell cells[8]; uint64_t info[8];
	CHECK(bh_site_counts_host(NULL, ranges, 5, sites, 1, alleles, 2, recs, 8, cells, info) == BH_OK && info[0] == 5 && info[1] == 8);
	CHECK(cell_is(&cells[0], 2, 0, 0, 0, 2, 0) && cell_is(&cells[1], 7, 7, 0, 0, 0, 0) && cell_is(&cells[2], 0, 0, 0, 0, 0, 0) && cell_is(&cells[3], 2, 0, 0, 2, 0, 0));
	CHECK(cell_is(&cells[4], 6, 1, 5, 0, 0, 0) && cell_is(&cells[5], 3, 3, 0, 0, 0, 0) && cell_is(&cells[6], 6, 0, 0, 0, 0, 1) && cell_is(&cells[7], 6, 0, 0, 0, 0, 0));
	CHECK(bh_site_counts_host(NULL, ranges, 0, sites, 1, alleles, 2, recs, 8, cells, NULL) == BH_OK && cell_is(&cells[4], 0, 1, 5, 0, 0, 0) && cell_is(&cells[6], 0, 0, 0, 0, 0, 1));
	CHECK(bh_site_counts_host(NULL, ranges, 5, sites, 1, alleles, 2, recs, 0, NULL, NULL) == BH_OK);
	BhipCountRange bad_r = {3, 0, 1, 1};
	CHECK(bh_site_counts_host(NULL, &bad_r, 1, NULL, 0, NULL, 0, recs, 1, cells, NULL) == BH_E_USAGE && strstr(bh_last_error(), "range 0"));
	BhipCountRecord bad_q = {3, 5, 0, 0, 0};
	CHECK(bh_site_counts_host(NULL, ranges, 5, NULL, 0, NULL, 0, &bad_q, 1, cells, NULL) == BH_E_USAGE && strstr(bh_last_error(), "ref 0"));
	const BhipAllele twice[2] = {alleles[0], alleles[0]};
	CHECK(bh_site_counts_host(NULL, ranges, 5, NULL, 0, twice, 2, recs, 1, cells, NULL) == BH_E_USAGE && strstr(bh_last_error(), "alleles not strictly ascending"));

	/* ---- the object: headers 0 beta, 1 alpha x, 2 gamma; thresholds (2, 2) ---- */
	char *prefix = NULL, *fin = NULL, *dir = argv[1], *o1 = NULL, *o3 = NULL, *o1v = NULL, *o3v = NULL;
	CHECK(asprintf(&prefix, "%s/P_", dir) > 0 && asprintf(&fin, "%sstudy.vcf", prefix) > 0 && asprintf(&o1, "%s/s1.b6", dir) > 0 && asprintf(&o3, "%s/s3.b6", dir) > 0);
	CHECK(asprintf(&o1v, "%s.vcf", o1) > 0 && asprintf(&o3v, "%s.vcf", o3) > 0);
	const char *clash[2] = {"a/s1.b6", "b/s1.txt"};
	CHECK(bh_vcfstudy_check_names(clash, 2) == BH_E_USAGE && strstr(bh_last_error(), "'a/s1.b6'") && strstr(bh_last_error(), "'b/s1.txt'"));
	BhVcfStudy *st = NULL;
	CHECK(bh_vcfstudy_open(prefix, &st) == BH_OK && st);
	bh_vcfstudy_set_solver(st, bh_site_counts_host, NULL);
	BhVcf *v = open_vcf(&R, st);
	CHECK(v);
	/* sample 1 -- beta: 1..8 twice, 9..16 once, 21..28 with three reads that show A at 24 and one that shows T; alpha x: both reads delete
	 * column 8; gamma: both reads insert G behind 4.  Sample 2 fails alone.  Sample 3: two plain reads on beta 21..28, nothing else */
	BhPathLine n1[] = {{0, 0, 0, 1}, {0, 0, 0, 1}, {1, 0, 0, 1}, {2, 0, 0, 1}, {2, 0, 0, 1}, {2, 0, 0, 1}, {3, 0, 0, 1}};
	BhPathLine n2[] = {{4, 4, 1, 1}, {4, 4, 1, 1}, {5, 0, 2, 0}, {5, 0, 2, 0}};
	BhPathBuf bufs[2] = {{n1, 7, 7}, {n2, 4, 4}};
	CHECK(bh_vcf_collect(v, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, bufs, 2) == BH_OK);
	CHECK(bh_vcf_sample(v, NULL, o1, q_codes, q_off, 4) == BH_OK);
	bh_vcf_print_info(v);
	CHECK(bh_vcf_collect(v, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, bufs, 2) == BH_OK);
	bh_vcf_sample_failed(v);
	CHECK(bh_vcf_study_sample_failed(v, "elsewhere/broken.b6") == BH_OK);
	BhPathLine n3[] = {{3, 0, 0, 1}, {3, 0, 0, 1}};
	BhPathBuf one = {n3, 2, 2};
	CHECK(bh_vcf_collect(v, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, &one, 1) == BH_OK);
	CHECK(bh_vcf_sample(v, NULL, o3, q_codes, q_off, 4) == BH_OK);
	CHECK(!slurp(fin));      /* nothing under the final name before the write */
	CHECK(bh_vcfstudy_write(st, v, NULL) == BH_OK);
	bh_vcfstudy_print_info(st);
	uint64_t fig[8];
	bh_vcfstudy_last_info(st, fig);
	CHECK(fig[0] == 2 && fig[1] == 1 && fig[2] == 1 && fig[3] == 1 && fig[4] == 1 && fig[5] == 6 && fig[6] > 0 && fig[7] == 0);
	CHECK(bh_vcfstudy_write(st, v, NULL) != BH_OK);      /* once */
	char *got = slurp(fin), *own1 = slurp(o1v), *own3 = slurp(o3v);
	CHECK(got && own1 && own3);
	CHECK(strstr(got, "##contig=<ID=gamma,length=8>\n##INFO=<ID=DP,") && strstr(got, "##INFO=<ID=NS,Number=1,Type=Integer,"));
	CHECK(strstr(got, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\tbroken\ts3\n"
	                  "beta\t24\t.\tT\tA\t.\t.\tDP=6;NS=2\tDP:AD\t4:1,3\t.\t2:2,0\n"
	                  "alpha\t7\t.\tGT\tG\t.\t.\tDP=2;NS=1\tDP:AD\t2:0,2\t.\t0:0,0\n"
	                  "gamma\t4\t.\tT\tTG\t.\t.\tDP=2;NS=1\tDP:AD\t2:0,2\t.\t0:0,0\n"));
	CHECK(strstr(own1, "\ts1\nbeta\t24\t.\tT\tA\t.\t.\tDP=4\tDP:AD\t4:1,3\nalpha\t7\t.\tGT\tG\t.\t.\tDP=2\tDP:AD\t2:0,2\ngamma\t4\t.\tT\tTG\t.\t.\tDP=2\tDP:AD\t2:0,2\n"));
	CHECK(strstr(own3, "\ts3\n") && !strstr(own3, "\nbeta\t"));      /* sample 3 reports nothing itself */
	free(got); free(own1); free(own3);
	bh_vcfstudy_close(st);
	bh_vcf_close(v);
	CHECK(!remove(fin) && !remove(o1v) && !remove(o3v));
	/* two samples of one name through the collector; an abort; the device solver without a handle; a close without a write */
	CHECK(bh_vcfstudy_open(prefix, &st) == BH_OK && (v = open_vcf(&R, st)));
	bh_vcfstudy_set_solver(st, bh_site_counts_host, NULL);
	CHECK(bh_vcf_collect(v, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, bufs, 2) == BH_OK && bh_vcf_sample(v, NULL, o1, q_codes, q_off, 4) == BH_OK);
	CHECK(bh_vcf_collect(v, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, bufs, 2) == BH_OK);
	CHECK(bh_vcf_sample(v, NULL, o1, q_codes, q_off, 4) == BH_E_USAGE && strstr(bh_last_error(), "both sample 's1'"));
	bh_vcf_abort(v);
	CHECK(bh_vcfstudy_write(st, v, NULL) != BH_OK && !slurp(fin));
	bh_vcfstudy_close(st); bh_vcf_close(v);
	CHECK(bh_vcfstudy_open(prefix, &st) == BH_OK && (v = open_vcf(&R, st)));      /* (the device) */
	CHECK(bh_vcf_collect(v, rec_idx, rec_req, rec_first, rec_off, rec_ops, 6, bufs, 2) == BH_OK && bh_vcf_sample(v, NULL, o1, q_codes, q_off, 4) == BH_OK);
	CHECK(bh_vcfstudy_write(st, v, NULL) == BH_E_DEVICE && strstr(bh_last_error(), "no device handle") && !slurp(fin));
	bh_vcfstudy_close(st); bh_vcf_close(v);
	CHECK(bh_vcfstudy_open(prefix, &st) == BH_OK);
	bh_vcfstudy_close(st);
	bh_vcfstudy_close(NULL);
	CHECK(!remove(o1v) && !slurp(fin));
	free(prefix); free(fin); free(o1); free(o3); free(o1v); free(o3v);
	puts("vcfstudy_host_main ok");
	return 0;
}
